"""What the depthwise row-stream launchers (crnn_dwconv3x3_{fwd,bwd}_stream*) answer when they refuse a call, and the sweep of their shape queries.

    python tests/golden/make_dw_stream_refusals.py <libcrnn_mi355x.so of the revision to record> [-o tests/golden/dw_stream_refusals.json]

Every pattern here is refused on the host BEFORE a launch -- a missing operand, a bad dtype / rate / out_order, an operand that is not 16-byte
aligned (keep bytes: 4-byte), a shape the query refuses -- so the operands are made-up addresses that nothing dereferences.  An operand the launchers
do not check for alignment (the statistics partials, dk, scratch) is never misaligned here: such a call would reach the launch.
tests/test_host_cpu.py replays the patterns on the built library against the recorded codes."""
import ctypes
import itertools
import json
import os
import sys

F32, BF16, BAD_DT = 0, 1, 7
GOOD = (2, 52, 9, 512)        # every form of both kernels takes it, in both storage types (checked by records())
REFUSED = (2, 13, 9, 64)      # no form takes it but the backward on fp32 maps (144 columns): left out there

# the queries' sweep
SWEEP_B, SWEEP_H = (1, 5, 64, 256), (1, 3, 8, 13, 52, 104, 204)
SWEEP_W, SWEEP_C = (1, 9, 17, 18, 26, 36, 52, 68), (1, 8, 64, 128, 252, 256, 512)
QUERIES = ["crnn_dwconv_%s_stream_%s" % (d, q) for d in ("fwd", "bwd") for q in ("supported", "rows", "pro_supported")]

# operand kinds -- A: required, 16-byte aligned; R: required; a: optional, 16-byte aligned when present; o: optional; K: keep bytes (4-byte aligned)
_FWD = [("x", "A"), ("k", "A"), ("out", "A"), ("stat_partials", "o")]
_FWD_PRO = [("q", "A"), ("pro_bnstate", "A"), ("rate", "rate"), ("keep", "K"), ("k", "A"), ("out", "A"), ("stat_partials", "o")]
_BWD = [("d", "A"), ("da", "A"), ("bnstate", "A"), ("coef", "A"), ("xin", "A"), ("k", "A"), ("dx", "A"), ("dk", "R"), ("scratch", "R")]
_BWD_PRO = [("d", "A"), ("da", "A"), ("bnstate", "A"), ("coef", "A"), ("q", "A"), ("pro_bnstate", "A"), ("rate", "rate"), ("keep", "K"), ("k", "A"),
            ("dx", "A"), ("dk", "R"), ("scratch", "R"), ("bn2_stat_partials", "o")]
_SHAPE = [("B", "int"), ("H", "int"), ("W", "int"), ("C", "int")]
LAUNCHERS = {
    "crnn_dwconv3x3_fwd_stream": _FWD + [("bnstate", "a")] + _SHAPE + [("flip", "int")],
    "crnn_dwconv3x3_fwd_stream_ex": _FWD + [("bnstate", "a")] + _SHAPE + [("flip", "int"), ("out_order", "int")],
    "crnn_dwconv3x3_fwd_stream_dt": _FWD + _SHAPE + [("flip", "int"), ("dtype", "int")],
    "crnn_dwconv3x3_fwd_stream_pro": _FWD_PRO + _SHAPE,
    "crnn_dwconv3x3_fwd_stream_pro_ex": _FWD_PRO + _SHAPE + [("dtype", "int")],
    "crnn_dwconv3x3_bwd_stream": _BWD + _SHAPE,
    "crnn_dwconv3x3_bwd_stream_ex": _BWD + _SHAPE + [("dtype", "int")],
    "crnn_dwconv3x3_bwd_stream_pro": _BWD_PRO + _SHAPE,
    "crnn_dwconv3x3_bwd_stream_pro_ex": _BWD_PRO + _SHAPE + [("dtype", "int")],
}


def load(path):
    """The library at `path` with the header's argument types (no torch: nothing here touches a device)."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(here)), "crnn-ocr-lite_amd"))
    from crnn_mi355x import native
    L = ctypes.CDLL(path)
    for name, (ret, args) in native.parse_header().items():
        if "dwconv" in name and "stream" in name:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ret, args
    return L


def patterns():
    """-> [(key, function, [arguments])]: every refusal pattern of every launcher (typed launchers: for both storage types)."""
    out = []
    for fn, sig in LAUNCHERS.items():
        names = [n for n, _ in sig]
        typed = "dtype" in names
        for dt in ((F32, BF16) if typed else (None,)):
            base = {}
            for i, (n, kind) in enumerate(sig):
                if kind in ("A", "R", "K"):
                    base[n] = 0x7f0000000000 + 0x1000000 * (i + 1)      # 16-byte aligned, never dereferenced
                elif kind in ("a", "o"):
                    base[n] = None
                elif kind == "rate":
                    base[n] = 0.1
            base.update(zip("BHWC", GOOD), flip=0, out_order=0, dtype=dt)

            def add(what, **change):
                args = dict(base, **change)
                out.append(("%s%s %s" % (fn, "" if dt is None else " dt%d" % dt, what), fn, [args[n] for n in names] + [None]))   # (+ the stream)
            for n, kind in sig:
                if kind in ("A", "R"):
                    add("null " + n, **{n: None})
                if kind == "A":
                    add("misaligned " + n, **{n: base[n] + 4})
                if kind == "a":
                    add("misaligned " + n, **{n: 0x7e0000000000 + 4})
                if kind == "K":
                    add("keep + 1", keep=base[n] + 1)
                    add("keep + 2", keep=base[n] + 2)
                    add("keep + 2 rate 0", keep=base[n] + 2, rate=0.0)
                    add("rate > 0 null keep", keep=None)
                if kind == "rate":
                    add("rate < 0", rate=-0.5)
                    add("rate 1", rate=1.0)
            if typed and dt == F32:
                add("bad dtype", dtype=BAD_DT)
            if "out_order" in names:
                add("out_order -1", out_order=-1)
                add("out_order 2", out_order=2)
                add("out_order 1 null bnstate", out_order=1)
                add("out_order 1 odd H", out_order=1, bnstate=0x7e0000000000, H=GOOD[1] + 1)
            if not ("_bwd_" in fn and dt == F32):
                add("refused shape", **dict(zip("BHWC", REFUSED)))
    return out


def sweep():
    return itertools.product(SWEEP_B, SWEEP_H, SWEEP_W, SWEEP_C)


def records(L):
    """-> {pattern key: return code}"""
    for q in QUERIES:
        if not q.endswith("rows"):
            assert all(getattr(L, q + "_ex")(*GOOD, dt) == 0 for dt in (F32, BF16)), q
            assert all(getattr(L, q + "_ex")(*REFUSED, dt) == -3 for dt in (F32, BF16) if not ("_bwd_" in q and dt == F32)), q
    return {key: getattr(L, fn)(*args) for key, fn, args in patterns()}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "dw_stream_refusals.json"))
    a = ap.parse_args()
    rec = records(load(a.lib))
    assert all(v in (-2, -3) for v in rec.values()), "a pattern was not refused: %s" % [k for k, v in rec.items() if v not in (-2, -3)]
    json.dump({"records": rec}, open(a.out, "w"), indent=0, sort_keys=True)
    print("%d patterns -> %s" % (len(rec), a.out))
