#!/usr/bin/env python3
"""Record the output bits of the plain beam-search decoder of the built library: tests/golden/beam_bits.npz.

crnn_ctc_beam_decode and crnn_ctc_beam_decode_lm run one kernel (csrc/beam.hip), so comparing the two entry points with each other cannot see a
mistake in it; this pins labels, lengths and score bits from outside.  Recorded from the last commit at which the plain decoder had a kernel of
its own.  Outputs only: the inputs are rebuilt from seeds (tests/lm_beam_ref.py).  Needs the MI355X; run it from the commit whose bits are to be
pinned:
    python tests/golden/make_beam_bits.py
tests/test_gpu_lm.py replays these inputs through both entry points and compares the raw bits with load().  The fixture holds for the compiler it
was recorded with: `hipcc --version` is stored beside the arrays."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), os.path.join(os.path.dirname(TESTS), "crnn-ocr-lite_amd"), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
import lm_beam_ref as R  # noqa: E402  (the inputs: plain_case_inputs, edge_inputs)
OUT = os.path.join(HERE, "beam_bits.npz")
MAX_BYTES = 300 * 1000

FILL_LABEL, FILL_LEN, FILL_SCORE = 1000, -5, 7.0          # none is a value a decode can write


def hipcc_version():
    try:
        return subprocess.run(["hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout.strip()
    except OSError as e:
        return "hipcc --version: %s" % e


def plain(y, il, bw, merge):
    """one call of crnn_ctc_beam_decode on ndarrays -> (labels (B, T) int32, lengths (B,) int32, score bits (B,) int32); outputs pre-filled"""
    import torch
    from gpu_util import L, dev, P, S, ok, host
    n, t, C = y.shape
    out = torch.full((n, t), FILL_LABEL, dtype=torch.int32, device="cuda")
    ln = torch.full((n,), FILL_LEN, dtype=torch.int32, device="cuda")
    sc = torch.full((n,), FILL_SCORE, device="cuda")
    ok(L().crnn_ctc_beam_decode(P(dev(y)), P(dev(il, np.int32)) if il is not None else None, P(out), P(ln), P(sc), n, t, C, bw, merge, S()))
    return host(out), host(ln), host(sc).view(np.int32)


def names(tag):
    return tuple("%s %s" % (k, tag) for k in ("labels", "lengths", "score bits"))


def case_tag(C, bw, merge):
    return "C%d width%d merge%d" % (C, bw, merge)


EDGE_TAG = "edge C%d T%d width%d merge%d" % (R.EDGE_C, R.EDGE_T, R.EDGE_BW, R.EDGE_MERGE)


def arrays():
    """{name: int32 ndarray} of every recorded output, computed with the built library on the current device"""
    out = {}
    for C, bw, merge in R.PLAIN_CASES:
        y, il = R.plain_case_inputs(C, bw)
        out.update(zip(names(case_tag(C, bw, merge)), plain(y, il, bw, merge)))
    out.update(zip(names(EDGE_TAG), plain(R.edge_inputs(), None, R.EDGE_BW, R.EDGE_MERGE)))
    return out


def load(path=OUT):
    """-> ({name: int32 ndarray} as arrays() returns it, the recorded `hipcc --version`); labels are stored as int8 (-1 .. 127)"""
    gold = np.load(path)
    return {k: gold[k].astype(np.int32) for k in gold.files if k != "hipcc_version"}, str(gold["hipcc_version"])


if __name__ == "__main__":
    if len(sys.argv) > 1:
        OUT = sys.argv[1]
    rec = arrays()
    assert len(rec) == 3 * (len(R.PLAIN_CASES) + 1)
    for name, a in rec.items():                               # nothing was left at its fill value, and what gets pinned has something to pin
        fill = FILL_LABEL if name.startswith("labels") else FILL_LEN if name.startswith("lengths") else np.float32(FILL_SCORE).view(np.int32)
        assert a.dtype == np.int32 and not (a == fill).any(), "an output was not written: %s" % name
        if name.startswith("labels"):
            assert a.min() == -1 and a.max() <= 127
    for C, bw, merge in R.PLAIN_CASES:
        assert (rec["lengths " + case_tag(C, bw, merge)][4:] > 5).all()
    assert (rec["lengths " + EDGE_TAG] > 100).all()
    keep = {k: (a.astype(np.int8) if k.startswith("labels") else a) for k, a in rec.items()}
    np.savez_compressed(OUT, hipcc_version=np.array(hipcc_version()), **keep)
    size = os.path.getsize(OUT)
    assert size < MAX_BYTES, "%s is %d bytes" % (OUT, size)
    back, _ = load(OUT)
    assert sorted(back) == sorted(rec) and all(np.array_equal(back[k], rec[k]) for k in rec)
    print("wrote", OUT, len(rec), "arrays,", size, "bytes")
