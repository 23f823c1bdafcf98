#!/usr/bin/env python3
"""Lexicon shortlists at batch 1024, T = 52 (the 100 x 32 configuration), 38 classes, by scripts/lexicon_bench.py's method: the posteriors of the benchmark
model (random weights) against the same seeded synthetic lexicons of 1 000 / 10 000 / 88 000 words; HIP events over windows of about 1 s of back-to-back
calls after warm-up; every lexicon size in a process of its own under its own time limit, two alternating runs of every figure; the first step that fails
ends the run.  Prints, and with --out writes,
  (a) crnn_lexicon_nearest alone (the clear of the histogram, the distance kernel and the selection kernel), K = 50, P = 1 and 3, queries = the beam paths:
      the product library and, where scripts/_trace/libnear_wpt<k>.so exist (scripts/build_nearest_variants.sh: -DNEAR_WORDS_PER_THREAD=k, a tile of 256 k
      words per workgroup), those builds -- their rows must equal the product's;
  (b) the whole shortlist decode, LexiconDecoder(shortlist=K, paths=P)._topk on the device map -- beam search, nearest, scores, top-1 -- for K = 16, 50, 200
      and P = 1, 3, next to the exhaustive decode LexiconDecoder()._topk of the same build in the same process (the baseline: without the shortlist the only
      way to a lexicon decode), and the ratio;
  (c) agreement with the exhaustive decoder, N = 10 000: the share of images on which both return the same word, on the benchmark model's posteriors (an
      untrained model: near-flat maps, which say little about a real recogniser -- no trained one is at hand) and on the constructed fixture of
      tests/nearest_ref.py scaled to 10 000 words and 1008 images;
and the kernels' resource usage as the compiler reports it.  usage: lexicon_shortlist_bench.py [--out FILE]"""
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from lexicon_bench import BATCH, T, C, BEAM, SIZES, make_lexicon, make_engine, _timed  # noqa: E402

KS, PS = (16, 50, 200), (1, 3)
NEAR_K = 50
AGREE_N, AGREE_IMAGES = 10000, 1008
STEPS = [("resources", 120)] + [("size%d" % n, 400) for n in SIZES] + [("agree", 400)]


def _events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _posteriors():
    eng, x = make_engine()
    y = eng.forward(x, train=False).float().contiguous()
    eng.check_rnn_status()
    return y


def _libs():
    import ctypes
    from crnn_mi355x import native
    out = [("product", native.lib())]
    for path in sorted(glob.glob(os.path.join(ROOT, "scripts", "_trace", "libnear_wpt*.so"))):
        lib = ctypes.CDLL(path)
        for name in ("crnn_lexicon_nearest", "crnn_lexicon_nearest_workspace_bytes"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = getattr(native.lib(), name).argtypes, getattr(native.lib(), name).restype
        out.append((os.path.basename(path)[7:-3], lib))
    return out


def _nearest_call(lib, paths, lab, ln, idx, dist, ws):
    import ctypes
    import torch
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    B, P, qcols = paths.shape
    N, Lmax = lab.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.crnn_lexicon_nearest(p(paths), P, qcols, p(lab), p(ln), p(idx), p(dist), p(ws), ws.numel() * 4, B, C, N, Lmax, idx.shape[1], st)
        assert rc == 0, rc
    return fn


def step_size(n_words):
    import torch
    from crnn_mi355x.engine import beam_decode_lm
    from crnn_mi355x.lexicon import LexiconDecoder
    y = _posteriors()
    lex = make_lexicon(n_words)
    lab, ln = lex.device(y.device)
    res = {"N": len(lex), "nearest_us": {}, "decode_us": {}, "exhaustive_us": []}
    paths = {p: beam_decode_lm(y, None, beam_width=BEAM, top_paths=p, merge_repeated=False)[0] for p in PS}
    decs = {(k, p): LexiconDecoder(lex, shortlist=k, paths=p, beam_width=BEAM) for k in KS for p in PS}
    full = LexiconDecoder(lex)
    want = full._topk(y, None, 1)[0].cpu().numpy()
    libs = _libs()
    idx = torch.empty((BATCH, NEAR_K), dtype=torch.int32, device="cuda"); dist = torch.empty_like(idx)
    ws = torch.empty(libs[0][1].crnn_lexicon_nearest_workspace_bytes(BATCH, len(lex)) // 4, dtype=torch.int32, device="cuda")
    for rnd in range(2):                                      # the figures alternate: what disturbs one window disturbs its neighbours
        for p in PS:
            first = None
            for name, lib in libs:
                us, _ = _timed(_nearest_call(lib, paths[p], lab, ln, idx, dist, ws), torch.cuda.synchronize, _events)
                res["nearest_us"].setdefault("P%d" % p, {}).setdefault(name, []).append(round(us, 1))
                got = (idx.cpu().numpy().copy(), dist.cpu().numpy().copy())
                first = first or got
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), "build %s selects differently" % name
        res["exhaustive_us"].append(round(_timed(lambda: full._topk(y, None, 1), torch.cuda.synchronize, _events)[0], 1))
        for (k, p), dec in decs.items():
            us, _ = _timed(lambda: dec._topk(y, None, 1), torch.cuda.synchronize, _events)
            res["decode_us"].setdefault("K%d_P%d" % (k, p), []).append(round(us, 1))
    res["agree"] = {"K%d_P%d" % kp: float((dec._topk(y, None, 1)[0].cpu().numpy() == want).mean()) for kp, dec in decs.items()}
    q = paths[1][:, 0].cpu().numpy()
    res["mean_query_len"] = float(((q >= 0) & (q <= C - 2)).sum(1).mean())
    return {"size%d" % n_words: res}


def step_agree():
    """The constructed fixture scaled up: every image spells a word of the table, a third with a substitution, a third with a deletion."""
    import torch
    import nearest_ref as NR
    from crnn_mi355x.lexicon import Lexicon, LexiconDecoder
    from crnn_mi355x import data as D
    ynp, words = NR.fixture(N=AGREE_N, images=AGREE_IMAGES)
    chars = list(D.get_lexicon())
    lex = Lexicon(["".join(chars[c] for c in w) for w in words], dict(enumerate(chars)))
    y = torch.from_numpy(np.array(ynp)).cuda()
    want = LexiconDecoder(lex)._topk(y, None, 1)[0].cpu().numpy()
    out = {}
    for k in KS:
        for p in PS:
            got = LexiconDecoder(lex, shortlist=k, paths=p, beam_width=BEAM)._topk(y, None, 1)[0].cpu().numpy()
            out["K%d_P%d" % (k, p)] = float((got == want).mean())
    return {"fixture_agree": out}


def step_resources():
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "lexicon_nearest.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out = {}
    for blk in err.split("Function Name: ")[1:]:
        name = blk.split()[0]
        pick = lambda key: int(re.search(r"%s: (\d+)" % re.escape(key), blk).group(1))
        out["dist" if "near_dist" in name else "select"] = {"vgprs": pick("VGPRs"), "sgprs": pick("TotalSGPRs"), "scratch": pick("ScratchSize [bytes/lane]"),
                                                            "occupancy": pick("Occupancy [waves/SIMD]"), "lds": pick("LDS Size [bytes/block]")}
    return {"resources": out}


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        step = sys.argv[2]
        res = step_size(int(step[4:])) if step.startswith("size") else {"resources": step_resources, "agree": step_agree}[step]()
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
    both = lambda us: " / ".join("%.1f" % u for u in us)
    lines = ["lexicon shortlists: batch %d, T = %d (100 x 32), %d classes; posteriors of the benchmark model (random weights: its beam paths have %.1f symbols on average);"
             % (BATCH, T, C, r["size%d" % SIZES[0]]["mean_query_len"]),
             "the seeded synthetic lexicons of scripts/lexicon_bench.py (lengths 2..23, sorted by length).  HIP events over windows of about 1 s of back-to-back calls after",
             "warm-up; every lexicon size in a process of its own; two alternating runs of every figure, both shown; ratios from the better run of each.", ""]
    for n in SIZES:
        d = r["size%d" % n]
        lines.append("  N = %6d words" % d["N"])
        for p in PS:
            for name, us in d["nearest_us"]["P%d" % p].items():
                lines.append("    (a) crnn_lexicon_nearest alone, K = %d, P = %d, %-8s %s us per call = %.3f us per image, %.3g (query, word) pairs/s"
                             % (NEAR_K, p, name + ":", both(us), min(us) / BATCH, BATCH * d["N"] * p / (min(us) * 1e-6)))
        ex = min(d["exhaustive_us"])
        lines.append("    (b) exhaustive decode (baseline, every word scored): %s us per batch = %.2f us per image" % (both(d["exhaustive_us"]), ex / BATCH))
        for k in KS:
            for p in PS:
                us = d["decode_us"]["K%d_P%d" % (k, p)]
                lines.append("        shortlist decode K = %3d, P = %d (beam + nearest + scores + top-1): %s us per batch = %.2f us per image: %.1f x the baseline's rate; same word as the baseline on %.1f %% of the images"
                             % (k, p, both(us), min(us) / BATCH, ex / min(us), 100 * d["agree"]["K%d_P%d" % (k, p)]))
    lines += ["", "  (c) agreement with the exhaustive decoder.  The percentages above are on the posteriors of an UNTRAINED model: near-flat maps on which the best word is",
              "      decided by length and chance letters, far from any decode -- they say little about a real recogniser, and no trained one is at hand.  On the constructed",
              "      fixture of tests/nearest_ref.py (every image spells a table word at 0.9 per frame; a third with one substitution, a third with one deletion) scaled to",
              "      N = %d words and %d images, the same word as the exhaustive decoder on: %s"
              % (AGREE_N, AGREE_IMAGES, "; ".join("K = %s, P = %s: %.1f %%" % (key.split("_")[0][1:], key.split("_")[1][1:], 100 * v) for key, v in r["fixture_agree"].items())),
              "      K = 50 stays a placeholder default: tune it on held-out data of the recogniser in use.", "",
              "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): " +
              "; ".join("%s %d VGPRs / %d SGPRs / %d B LDS / scratch %d / occupancy %d" % (k, v["vgprs"], v["sgprs"], v["lds"], v["scratch"], v["occupancy"])
                        for k, v in sorted(r["resources"].items()))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
