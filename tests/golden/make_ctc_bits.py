#!/usr/bin/env python3
"""Record the output bits of the softmax / CTC entry points of the built library: tests/golden/ctc_bits.npz.

The loss, lexicon and alignment kernels share their arithmetic (csrc/ctc_core.h), so the tests that compare them with each other cannot see a
mistake they share; this pins every result from outside.  Outputs only: the inputs are rebuilt from seeds (tests/lexicon_ref.py).  Needs the
MI355X; run it from the commit whose bits are to be pinned:
    python tests/golden/make_ctc_bits.py
tests/test_gpu_ctc_bits.py recomputes arrays() with the library under test and compares the raw bits.  The fixture holds for the compiler it
was recorded with: `hipcc --version` is stored beside the arrays."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ctc_bits.npz")
MAX_BYTES = 300 * 1000

CLASSES = (38, 64, 65, 128)            # one class per lane up to 64, two from 65: both instantiations, both sides of the boundary
T, B, LMAX = 20, 6, 31
SKIPS = (0, 2)
SAMPLE_WORD_LENGTHS = (0, 1, 31, 7, 8, 15)      # one word per sample of posteriors(), for the loss and the alignment
CANDIDATES = np.array([[3, 17, 39, 0, 8], [-1, 5, -1, 5, 12], [-1, -1, -1, -1, -1], [40, 1, 1000000, -7, 2], [39, -1, -1, -1, -1],
                       [0, 1, 2, 3, -1]], dtype=np.int32)


def hipcc_version():
    try:
        return subprocess.run(["hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout.strip()
    except OSError as e:
        return "hipcc --version: %s" % e


def bits(a):
    """float32 -> its int32 bit patterns (NaN payloads and the sign of zero included); integers as they are"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _softmax(out, C):
    import torch
    from gpu_util import L, dev, P, S, ok, host
    rs = np.random.RandomState(7000 + C)
    rows = B                                                  # 6 rows: a whole workgroup of 4 and a partial one
    z = (rs.normal(size=(rows, C + 7)) * 3).astype(np.float32)
    bias = rs.normal(size=C).astype(np.float32)
    p = torch.full((rows, C), 7.0, device="cuda")
    ok(L().crnn_softmax_rows(P(dev(z[:, :C])), P(p), rows, C, S()))
    out["softmax_rows C%d" % C] = host(p)
    for ldz in (C, C + 7):
        zl = z[:, :ldz].copy()
        zl[:, C:] = np.nan                                    # padding columns are never read
        for permP in (0, 3):
            lg, p1, p2 = (torch.full((rows, C), 7.0, device="cuda") for _ in range(3))
            ok(L().crnn_softmax_rows_perm(P(dev(zl)), ldz, P(dev(bias)), P(lg), P(p1), P(p2), rows, C, permP, S()))
            for name, t in (("logits", lg), ("p1", p1), ("p2", p2)):
                out["softmax_rows_perm C%d ldz%d perm%d %s" % (C, ldz, permP, name)] = host(t)


def _ctc(out, C):
    import torch
    from gpu_util import L, dev, P, S, ok, host
    from lexicon_ref import posteriors, input_lengths, make_words, table, SEGMENT_LENGTHS
    y = np.array(posteriors(C, T))
    assert y.shape == (B, T, C)
    yd = dev(y)
    sample_words = make_words(C, n=B, seed=1, lengths=SAMPLE_WORD_LENGTHS)
    words = make_words(C, n=40)
    assert sorted(set(len(w) for w in words)) == sorted(SEGMENT_LENGTHS)
    wlab, wlen = table(words, width=LMAX)
    for skip in SKIPS:
        il = dev(input_lengths(T, skip), np.int32)
        tag = "C%d skip%d" % (C, skip)
        # loss and gradient (the loss kernel does not validate labels: padding is the blank, as engine.py uploads it)
        lab, ll = table(sample_words, width=LMAX, pad=C - 1)
        loss = torch.full((B,), 7.0, device="cuda"); dl = torch.full((T, B, C), 7.0, device="cuda")
        ok(L().crnn_ctc_loss_grad(P(yd), P(dev(lab, np.int32)), P(il), P(dev(ll, np.int32)), P(loss), P(dl), B, T, C, LMAX, skip, 1.0 / B, S()))
        out["loss %s" % tag] = host(loss)
        out["dlogits %s" % tag] = host(dl)
        # lexicon scores, dense and through candidate lists; the best 3 of the dense ones
        nbytes = L().crnn_ctc_lexicon_workspace_bytes(B, T, C, skip)
        assert nbytes == B * (T - skip) * C * 4
        wl, wn = dev(wlab, np.int32), dev(wlen, np.int32)
        for cand in (None, CANDIDATES):
            M = 40 if cand is None else cand.shape[1]
            sc = torch.full((B, M), 7.0, device="cuda"); ws = torch.full((nbytes // 4,), 7.0, device="cuda")
            ok(L().crnn_ctc_lexicon_score(P(yd), P(il), P(wl), P(wn), P(dev(cand, np.int32)) if cand is not None else None, P(sc), P(ws), nbytes,
                                          B, T, C, skip, 40, LMAX, 0 if cand is None else M, S()))
            out["lexicon %s %s" % ("dense" if cand is None else "candidates", tag)] = host(sc)
            if cand is None:
                idx = torch.full((B, 3), 77, dtype=torch.int32, device="cuda"); val = torch.full((B, 3), 7.0, device="cuda")
                ok(L().crnn_ctc_lexicon_topk(P(sc), None, P(idx), P(val), B, 40, 3, S()))
                out["topk idx %s" % tag] = host(idx)
                out["topk val %s" % tag] = host(val)
        # alignment: the five outputs and the workspace
        lab, ll = table(sample_words, width=LMAX)
        res = {"score": torch.full((B,), 7.0, device="cuda"), "states": torch.full((B, T - skip), 77, dtype=torch.int32, device="cuda"),
               "start": torch.full((B, LMAX), 77, dtype=torch.int32, device="cuda"), "end": torch.full((B, LMAX), 77, dtype=torch.int32, device="cuda"),
               "char_logp": torch.full((B, LMAX), 7.0, device="cuda")}
        assert L().crnn_ctc_align_workspace_bytes(B, T, C, skip) == nbytes
        ws = torch.full((nbytes // 4,), 7.0, device="cuda")
        ok(L().crnn_ctc_align(P(yd), P(il), P(dev(lab, np.int32)), P(dev(ll, np.int32)), P(res["score"]), P(res["states"]), P(res["start"]),
                              P(res["end"]), P(res["char_logp"]), P(ws), nbytes, B, T, C, skip, LMAX, S()))
        for k, t in res.items():
            out["align %s %s" % (k, tag)] = host(t)
        out["align workspace %s" % tag] = host(ws).reshape(B, T - skip, C)
    # the decoders on the same maps (beam.hip shares only the two constants' names)
    il = dev(input_lengths(T, 0), np.int32)
    o = torch.full((B, T), 77, dtype=torch.int32, device="cuda"); n = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    ok(L().crnn_ctc_greedy_decode(P(yd), P(il), P(o), P(n), B, T, C, S()))
    out["greedy out C%d" % C] = host(o); out["greedy len C%d" % C] = host(n)
    o = torch.full((B, T), 77, dtype=torch.int32, device="cuda"); n = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    sc = torch.full((B,), 7.0, device="cuda")
    ok(L().crnn_ctc_beam_decode(P(yd), P(il), P(o), P(n), P(sc), B, T, C, 5, 1, S()))
    out["beam out C%d" % C] = host(o); out["beam len C%d" % C] = host(n); out["beam score C%d" % C] = host(sc)


def arrays():
    """{name: ndarray} of every recorded output, computed with the built library on the current device"""
    out = {}
    for C in CLASSES:
        _softmax(out, C)
        _ctc(out, C)
    return out


def _copy_of(name):
    """Outputs that are bit-copies of another by construction -- p2 of p1; the skip-2 workspace of frames 2.. of the skip-0 one (the pre-pass
    works row by row) -- are checked when the file is written and left out of it: -> (the other's name, index into it) or None"""
    if name.endswith(" p2"):
        return name[:-1] + "1", np.s_[:]
    if name.startswith("align workspace") and name.endswith("skip2"):
        return name[:-1] + "0", np.s_[:, 2:]
    return None


def load(path=OUT):
    """-> ({name: ndarray} as arrays() returns it, the recorded `hipcc --version`)"""
    gold = np.load(path)
    out = {k: gold[k] for k in gold.files if k not in ("names", "hipcc_version")}
    for name in gold["names"].tolist():
        if name not in out:
            src, idx = _copy_of(name)
            out[name] = out[src][idx]
    return out, str(gold["hipcc_version"])


if __name__ == "__main__":
    tests = os.path.dirname(HERE)
    for p in (os.path.join(os.path.dirname(tests), "crnn-ocr-lite_amd"), tests):
        sys.path.insert(0, p)
    rec = arrays()
    for C in CLASSES:                                          # what gets pinned has something to pin, and nothing was left at its fill value
        for skip in SKIPS:
            tag = "C%d skip%d" % (C, skip)
            loss, dense, score = rec["loss %s" % tag], rec["lexicon dense %s" % tag], rec["align score %s" % tag]
            assert np.isfinite(loss).sum() >= 2 and np.isinf(loss).sum() >= 2 and (rec["dlogits %s" % tag] != 0).any()
            assert np.isfinite(dense).any() and np.isneginf(dense).any() and np.isfinite(score).any() and np.isneginf(score).any()
            assert np.isfinite(rec["align workspace %s" % tag]).all()
        assert (rec["beam len C%d" % C] > 0).any() and (rec["greedy len C%d" % C] > 0).any()
    assert not any((a == 7.0).any() for k, a in rec.items() if a.dtype == np.float32 and not k.endswith(" logits")), "an output was not written"
    keep = {}
    for name, a in rec.items():
        if _copy_of(name) is None:
            keep[name] = a
        else:
            src, idx = _copy_of(name)
            assert np.array_equal(bits(a), bits(rec[src][idx])), name
    np.savez_compressed(OUT, hipcc_version=np.array(hipcc_version()), names=np.array(sorted(rec)), **keep)
    size = os.path.getsize(OUT)
    assert size < MAX_BYTES, "%s is %d bytes" % (OUT, size)
    back, _ = load()
    assert sorted(back) == sorted(rec) and all(np.array_equal(bits(back[k]), bits(rec[k])) for k in rec)
    print("wrote", OUT, len(rec), "arrays,", len(keep), "stored,", size, "bytes")
