#!/usr/bin/env python3
"""Lexicon decoding at batch 1024, T = 52 (the 100 x 32 configuration), 38 classes: crnn_ctc_lexicon_score + crnn_ctc_lexicon_topk (csrc/lexicon.hip) on the
posteriors of the benchmark model (random weights, as bench.predict_leg builds it) against seeded synthetic lexicons (lengths 2..23, weighted towards 5..10,
sorted by length as crnn_mi355x.lexicon.Lexicon uploads them).  Prints, and with --out writes,
  (a) dense scoring, N = 1 000 / 10 000 / 88 000 words: pairs/s and us per image for scoring + top-1, by HIP events, two alternating runs of every build:
      the product library and, where scripts/_trace/liblex_pack<k>.so exist (scripts/build_lexicon_variants.sh: -DLEX_PACK=k), the packing variants;
  (b) K = 50 candidates per image;
  (c) the kernels' own durations and the pre-pass's share, from a rocprofv3 --kernel-trace --stats run of its own;
  (d) the baseline -- the only way to the same numbers without this kernel: crnn_ctc_loss_grad over replicated posterior rows, one row per pair, N = 1 000
      in chunks of 16 images x 1 000 words (the replication itself is not timed);
  (e) context: forward + beam search (width 10) next to forward + lexicon decoding on the same engine;
and the kernels' resource usage as the compiler reports it.  Every figure is a child process of its own under its own time limit; the first one that fails
ends the run.  usage: lexicon_bench.py [--out FILE]"""
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np  # noqa: E402

BATCH, T, C, BEAM = 1024, 52, 38, 10
SIZES = (1000, 10000, 88000)
CAND_K = 50
STEPS = [("resources", 120), ("dense1000", 240), ("dense10000", 240), ("dense88000", 400), ("cand", 240), ("trace", 400), ("baseline", 300), ("context", 400)]
WINDOW_S = 1.0


def make_lexicon(n, seed=0):
    from crnn_mi355x import data as D
    from crnn_mi355x.lexicon import Lexicon
    rs = np.random.RandomState(seed)
    chars = np.array(list(D.get_lexicon()))
    lens = np.arange(2, 24)
    w = np.where((lens >= 5) & (lens <= 10), 6.0, 1.0)
    L = rs.choice(lens, size=n, p=w / w.sum())
    return Lexicon(["".join(chars[rs.randint(0, len(chars), size=l)]) for l in L], {i: ch for i, ch in enumerate(chars)})


def make_engine():
    """The benchmark model with non-degenerate random weights (bench.predict_leg) and one batch of its input."""
    import torch
    from bench import synthetic_batch
    from crnn_mi355x.engine import Engine
    from crnn_mi355x.init import initial_parameters
    eng = Engine(BATCH, dropout=False, precision="bf16s")
    p = initial_parameters(eng.layout, eng.cfg.units, False, seed=1)
    rs = np.random.RandomState(2)
    for k in p:
        if k.endswith(("_b", "_g")) or k == "stn_d2_w":
            p[k] = (p[k] + rs.normal(size=p[k].shape) * (0.02 if k.startswith("stn_d2") else 0.3)).astype(np.float32)
    eng.set_params(p)
    x, _, _, _ = synthetic_batch(BATCH, seed=0, T=eng.T)
    return eng, torch.from_numpy(x).cuda()


def _libs():
    import ctypes
    from crnn_mi355x import native
    out = [("product", native.lib())]
    for path in sorted(glob.glob(os.path.join(ROOT, "scripts", "_trace", "liblex_pack*.so"))):
        lib = ctypes.CDLL(path)
        for name in ("crnn_ctc_lexicon_score", "crnn_ctc_lexicon_topk"):
            getattr(lib, name).argtypes = getattr(native.lib(), name).argtypes
        out.append((os.path.basename(path)[6:-3], lib))
    return out


def wave_steps(lengths, pack=2, wpw=16):
    """Recursion steps one sample costs, in units of (one wave x one frame), by the packing rule of lex_score_kernel: a wave walks `wpw` consecutive
    words and takes four at a time where all have L <= 7, two where both have L <= 15, else one."""
    steps = 0
    for lo in range(0, len(lengths), wpw):
        seg = lengths[lo:lo + wpw]
        j = 0
        while j < len(seg):
            if pack >= 2 and j + 3 < len(seg) and max(seg[j:j + 4]) <= 7:
                j += 4
            elif pack >= 1 and j + 1 < len(seg) and max(seg[j:j + 2]) <= 15:
                j += 2
            else:
                j += 1
            steps += 1
    return steps


def _timed(fn, sync, events, window=None):
    """Warm-up, then us per call over a window of about WINDOW_S seconds of back-to-back calls, by HIP events."""
    for _ in range(3):
        fn()
    sync()
    t = time.time()
    fn(); sync()
    calls = max(3, int((window or WINDOW_S) / max(time.time() - t, 1e-6)))
    e0, e1 = events()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1) * 1e3 / calls, calls


def _scoring(n_words, k_cand, window=None):
    import ctypes
    import torch
    eng, x = make_engine()
    y = eng.forward(x, train=False).float().contiguous()
    eng.check_rnn_status()
    lex = make_lexicon(n_words)
    lab, ln = lex.device(y.device)
    N, Lmax = lab.shape
    M = k_cand or N
    cand = None
    if k_cand:
        cand = torch.from_numpy(np.sort(np.random.RandomState(1).randint(0, N, size=(BATCH, k_cand)).astype(np.int32), 1)).cuda()      # ascending, as LexiconDecoder passes them
    scores = torch.empty((BATCH, M), dtype=torch.float32, device="cuda")
    idx = torch.empty((BATCH, 1), dtype=torch.int32, device="cuda"); val = torch.empty((BATCH, 1), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    res, first = {}, None
    libs = _libs()
    ws = torch.empty(libs[0][1].crnn_ctc_lexicon_workspace_bytes(BATCH, T, C, 0) // 4, dtype=torch.float32, device="cuda")

    def call(lib):
        def fn():
            rc = lib.crnn_ctc_lexicon_score(p(y), None, p(lab), p(ln), p(cand), p(scores), p(ws), ws.numel() * 4, BATCH, T, C, 0, N, Lmax, k_cand, st)
            rc = rc or lib.crnn_ctc_lexicon_topk(p(scores), p(cand), p(idx), p(val), BATCH, M, 1, st)
            assert rc == 0, rc
        return fn
    for rnd in range(2):                                      # the builds alternate: what disturbs one window disturbs its neighbour
        for name, lib in libs:
            us, calls = _timed(call(lib), torch.cuda.synchronize, events, window)
            res.setdefault(name, []).append(round(us, 1))
            got = (idx.cpu().numpy().copy(), val.cpu().numpy().copy())
            first = first or got
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), "build %s decodes differently" % name
    lens = lex.lengths
    return {"us": res, "N": N, "M": M, "calls": calls, "steps": {"_pack%d" % k: wave_steps(lens.tolist(), k) for k in (0, 1, 2)} if not k_cand else None, "mean_len": float(lens.mean()), "share_le7": float((lens <= 7).mean()), "share_le15": float((lens <= 15).mean()),
            "finite_share": float(torch.isfinite(scores).float().mean()), "mean_best": float(val.mean())}


def step_resources():
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "lexicon.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out = {}
    for blk in err.split("Function Name: ")[1:]:
        name = blk.split()[0]
        pick = lambda key: int(re.search(r"%s: (\d+)" % re.escape(key), blk).group(1))
        short = "score" if "lex_score" in name else "topk" if "lex_topk" in name else "lsm2" if "ILi2" in name else "lsm1"
        out[short] = {"vgprs": pick("VGPRs"), "sgprs": pick("TotalSGPRs"), "scratch": pick("ScratchSize [bytes/lane]"), "occupancy": pick("Occupancy [waves/SIMD]")}
    return {"resources": out}


def step_trace():
    """The scoring steps again under rocprofv3 --kernel-trace --stats (a run of its own) -> mean duration of each kernel, dense N = 10 000 and K = 50."""
    import csv
    import tempfile
    out = {}
    for tag, step in (("dense", "dense10000"), ("cand", "cand")):
        folder = tempfile.mkdtemp()
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", folder, "-o", "lex", "--", sys.executable, os.path.abspath(__file__),
                        "--step", step, "--window", "0.2", "--product-only"], capture_output=True, text=True, check=True)
        for path in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in ("lex_lsm", "lex_score", "lex_topk"):
                    if key in row["Name"]:
                        out["trace_%s_%s_us" % (tag, key[4:])] = round(float(row["AverageNs"]) / 1e3, 2)
        if len([k for k in out if k.startswith("trace_" + tag)]) != 3:
            raise RuntimeError("kernel statistics not found under %s" % folder)
    return out


def step_baseline():
    """crnn_ctc_loss_grad over replicated rows: 16 images x 1 000 words per launch, 64 launches for the batch of 1024."""
    import ctypes
    import torch
    from crnn_mi355x import native
    eng, x = make_engine()
    y = eng.forward(x, train=False).float().contiguous()
    lex = make_lexicon(1000)
    N, Lmax = lex.labels.shape
    rows = 16 * N
    yrep = y[:16].repeat_interleave(N, 0).contiguous()
    lab = torch.from_numpy(np.where(lex.labels < 0, C - 1, lex.labels).astype(np.int32)).cuda().repeat(16, 1).contiguous()
    ll = torch.from_numpy(lex.lengths).cuda().repeat(16).contiguous()
    il = torch.full((rows,), T, dtype=torch.int32, device="cuda")
    loss = torch.empty(rows, device="cuda"); dl = torch.empty((T, rows, C), device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = native.lib()

    def batch():
        for _ in range(BATCH // 16):
            rc = L.crnn_ctc_loss_grad(p(yrep), p(lab), p(il), p(ll), p(loss), p(dl), rows, T, C, Lmax, 0, ctypes.c_float(1.0), st)
            assert rc == 0, rc
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    runs = [_timed(batch, torch.cuda.synchronize, events)[0] for _ in range(2)]
    # the same pairs by the new kernel, for the check that both compute the same thing
    lab2, ln2 = lex.device(y.device)
    scores = torch.empty((16, N), device="cuda")
    ws = torch.empty(L.crnn_ctc_lexicon_workspace_bytes(16, T, C, 0) // 4, device="cuda")
    rc = L.crnn_ctc_lexicon_score(p(y[:16].contiguous()), None, p(lab2), p(ln2), None, p(scores), p(ws), ws.numel() * 4, 16, T, C, 0, N, Lmax, 0, st)
    assert rc == 0, rc
    a, b = scores.reshape(-1).cpu().numpy(), -loss.cpu().numpy()
    fin = np.isfinite(b)
    assert np.array_equal(np.isneginf(a), np.isneginf(b)) and np.allclose(a[fin], b[fin], rtol=1e-6, atol=0)
    return {"baseline_us": [round(r, 1) for r in runs], "baseline_bit_identical": bool(np.array_equal(a, b))}


def step_context():
    import torch
    from crnn_mi355x.lexicon import lexicon_scores, lexicon_topk
    eng, x = make_engine()
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    out = {}
    lexs = {n: make_lexicon(n).device("cuda") for n in SIZES[:2]}

    def beam():
        eng.beam_decode(eng.forward(x, train=False), beam_width=BEAM)

    def lexicon(n):
        def fn():
            lab, ln = lexs[n]
            lexicon_topk(lexicon_scores(eng.forward(x, train=False).float(), lab, ln), 1)
        return fn
    out["forward_us"] = round(_timed(lambda: eng.forward(x, train=False), torch.cuda.synchronize, events)[0], 1)
    for rnd in range(2):
        out.setdefault("forward_beam_us", []).append(round(_timed(beam, torch.cuda.synchronize, events)[0], 1))
        for n in lexs:
            out.setdefault("forward_lexicon_%d_us" % n, []).append(round(_timed(lexicon(n), torch.cuda.synchronize, events)[0], 1))
    eng.check_rnn_status()
    return out


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        window = float(sys.argv[sys.argv.index("--window") + 1]) if "--window" in sys.argv else None
        if "--product-only" in sys.argv:
            global _libs
            from crnn_mi355x import native
            _libs = lambda: [("product", native.lib())]
        step = sys.argv[2]
        if step.startswith("dense"):
            res = {step: _scoring(int(step[5:]), 0, window)}
        elif step == "cand":
            res = {"cand": _scoring(SIZES[1], CAND_K, window)}
        else:
            res = {"resources": step_resources, "trace": step_trace, "baseline": step_baseline, "context": step_context}[step]()
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
        print("step %s done: %s" % (step, lines[-1][7:]), file=sys.stderr, flush=True)
    d = r["dense%d" % SIZES[0]]
    lines = ["lexicon decoding: batch %d, T = %d (100 x 32), %d classes; posteriors of the benchmark model (random weights); seeded synthetic lexicons, lengths 2..23" % (BATCH, T, C),
             "(mean %.1f; %.0f %% of the words have L <= 7, %.0f %% L <= 15), sorted by length.  HIP events over windows of about %.0f s of back-to-back calls after warm-up;"
             % (d["mean_len"], 100 * d["share_le7"], 100 * d["share_le15"], WINDOW_S),
             "every figure from a process of its own; two alternating runs of every build, both shown.  One call = pre-pass + scoring + top-1.", ""]
    for n in SIZES:
        d = r["dense%d" % n]
        lines.append("  (a) dense, N = %6d words (%.0f %% of the pairs have a path):" % (d["N"], 100 * d["finite_share"]))
        for name, us in d["us"].items():
            best = min(us)
            steps = d["steps"]["_pack2" if name == "product" else name]
            lines.append("        %-8s %12s us per call = %7.2f us per image, %.3g pairs/s; %d wave-steps per image and frame: %.0f cycles per wave-step and SIMD at the nominal 2.4 GHz"
                         % (name, " / ".join("%.1f" % u for u in us), best / BATCH, BATCH * d["N"] / (best * 1e-6), steps, 1024 * 2.4e3 * best / (BATCH * steps * (T - 1))))
    d = r["cand"]
    lines.append("  (b) K = %d candidates per image out of %d words:" % (CAND_K, d["N"]))
    for name, us in d["us"].items():
        lines.append("        %-8s %12s us per call = %7.3f us per image, %.3g pairs/s" % (name, " / ".join("%.1f" % u for u in us), min(us) / BATCH, BATCH * CAND_K / (min(us) * 1e-6)))
    for tag, what in (("dense", "dense N = %d" % SIZES[1]), ("cand", "K = %d" % CAND_K)):
        a, b, c = (r["trace_%s_%s_us" % (tag, k)] for k in ("lsm", "score", "topk"))
        lines.append("  (c) kernels alone, rocprofv3 --kernel-trace, %s: pre-pass %.1f us, scoring %.1f us, top-1 %.1f us: the pre-pass is %.1f %% of the three"
                     % (what, a, b, c, 100 * a / (a + b + c)))
    prod = min(r["dense%d" % SIZES[0]]["us"]["product"])
    base = min(r["baseline_us"])
    lines += ["  (d) baseline, N = %d: crnn_ctc_loss_grad over replicated rows (64 launches of 16 000 rows; replication not timed): %s us per batch = %.3g pairs/s;"
              % (SIZES[0], " / ".join("%.1f" % u for u in r["baseline_us"]), BATCH * SIZES[0] / (base * 1e-6)),
              "      the new kernels: %.1f us -> %.1f x; scores bit-identical to -loss on the 16 000 pairs compared: %s" % (prod, base / prod, r["baseline_bit_identical"]),
              "  (e) context, same engine (bf16s): forward %.1f us; forward + beam search (width %d) %s us; forward + lexicon decoding %s"
              % (r["forward_us"], BEAM, " / ".join("%.1f" % u for u in r["forward_beam_us"]),
                 "; ".join("N = %d: %s us" % (n, " / ".join("%.1f" % u for u in r["forward_lexicon_%d_us" % n])) for n in SIZES[:2])), "",
             "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): " +
             "; ".join("%s %d VGPRs / %d SGPRs / scratch %d / occupancy %d" % (k, v["vgprs"], v["sgprs"], v["scratch"], v["occupancy"]) for k, v in sorted(r["resources"].items()))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
