"""What the launchers of the step driver's streamed / weights-resident GEMMs and of the one-pass dropout answer when they refuse a call.

    python tests/golden/make_stream_gemm_refusals.py <libcrnn_mi355x.so of the revision to record> [-o tests/golden/stream_gemm_refusals.json]

Recorded from the library BEFORE every launcher's shape rule became one query (the launchers exist there, the whole-rule queries do not).  Every pattern is
refused on the host BEFORE a launch -- a missing operand, an operand that is not 16-byte aligned, or ONE violation of the shape / leading-dimension / row-offset /
scratch-size rule around an argument set the launcher accepts -- so the operands are made-up addresses that nothing dereferences.  The accepted sets are the
model's own calls at the benchmarked shape (100x32, batch 256, tds 128, 256 units: T*B = 13312 rows) and, where a kernel takes them, at the small test model
(40x32, batch 4, tds 32, 64 units); they are never passed to a launcher unperturbed.  An operand a launcher does not check (null or alignment) is never
perturbed that way: such a call would reach the launch.  tests/test_host_cpu.py replays the patterns on the built library against the recorded codes and asks
the whole-rule queries about every rule violation and every accepted set."""
import ctypes
import json
import os
import sys

MiB64 = 64 << 20
TB, G, FEAT = 13312, 1024, 4608     # the benchmarked shape: rows of the layers above the conv stack, LSTM gate columns, dense1's input features

# operand kinds -- A: required, 16-byte aligned; U: 16-byte aligned, presence not checked; R: required, any address; a: optional, aligned when present
_NT = [("A0", "A"), ("W0", "A"), ("A1", "a"), ("W1", "a"), ("Y", "A")]
_NT_SHAPE = ["M", "N", "K", "lda", "ldw", "ldy"]
_TN = lambda kind: [("A", kind), ("lda", None), ("B", kind), ("ldb", None), ("C", kind), ("ldc", None), ("M", None), ("N", None), ("K", None), ("scratch", "A"), ("scratch_bytes", None)]
_TN_SHAPE = ["M", "N", "K", "lda", "ldb", "ldc", "scratch_bytes"]
_BN3 = [("dq", "U"), ("W", "U"), ("da", "U"), ("M", None), ("N", None), ("K", None), ("d", "A"), ("bnstate", "A"), ("stat_partials", "R")]


def _ld_rules(names, mult):
    """one violation per leading dimension: below the extent it strides ("lda<M": lda = M - mult), and no multiple of `mult`"""
    return [("%s short" % n[:3], {n[:3]: ("below", n[4], mult)}) for n in names] + [("%s %% %d" % (n[:3], mult), {n[:3]: ("+", mult // 2)}) for n in names]


# launcher -> (arguments, whole-rule query, its arguments, accepted sets, rule violations {name: value | ("+", delta) | ("below", extent, delta)}, argument errors)
LAUNCHERS = {
    "crnn_gemm_wres_bf16": (
        [("X", "U"), ("W", "U"), ("Y", "U"), ("M", None), ("N", None), ("K", None)], "crnn_gemm_wres_bf16_supported", ["M", "N", "K"],
        [dict(M=958464, N=128, K=64), dict(M=119808, N=512, K=512), dict(M=TB, N=FEAT, K=128), dict(M=1584, N=256, K=256)],
        [("N % 128", {"N": ("+", 64)}), ("N 1152", {"N": 1152, "K": 256}), ("K 96", {"K": 96}), ("K 1024", {"K": 1024}), ("row offsets", {"M": 1 << 22, "N": 512, "K": 512})],
        [("M 0", {"M": 0}), ("N 0", {"N": 0}), ("K 0", {"K": 0})]),
    "crnn_pwconv_fwd_wres_folded": (
        [("a", "U"), ("wT", "U"), ("y", "U"), ("M", None), ("N", None), ("K", None), ("out_bnstate", "A")], "crnn_gemm_wres_bf16_supported", ["M", "N", "K"],
        [dict(M=958464, N=128, K=64), dict(M=119808, N=512, K=512), dict(M=1584, N=256, K=256)],
        [("N % 128", {"N": ("+", 64)}), ("N 1152", {"N": 1152, "K": 256}), ("K 96", {"K": 96}), ("row offsets", {"M": 1 << 22, "N": 512, "K": 512}), ("M 2^31", {"M": 1 << 31})],
        [("M 0", {"M": 0}), ("K 0", {"K": 0})]),
    "crnn_gemm_wres_bf16_bnstats": (
        [("X", "U"), ("W", "U"), ("Y", "U"), ("M", None), ("N", None), ("K", None), ("d", "A"), ("bnstate", "A"), ("stat_partials", "A")], "crnn_gemm_wres_bnstats_supported",
        ["M", "N", "K"], [dict(M=239616, N=256, K=256), dict(M=119808, N=512, K=512)],
        [("M % 128", {"M": ("+", 64)}), ("K 128", {"K": 128}), ("N % 128", {"N": ("+", 64)}), ("row offsets", {"M": 1 << 22, "N": 512, "K": 512}), ("M 0", {"M": 0})], []),
    "crnn_gemm_nt_bf16": (
        [("X", "U"), ("W", "U"), ("Y", "U"), ("M", None), ("N", None), ("K", None)], "crnn_gemm_nt_bf16_supported", ["M", "N", "K"],
        [dict(M=958464, N=128, K=256), dict(M=119808, N=512, K=512), dict(M=1584, N=256, K=256)],
        [("N % 128", {"N": ("+", 64)}), ("K % 64", {"K": ("+", 32)}), ("row offsets", {"M": 1 << 22, "N": 512, "K": 512})], [("M 0", {"M": 0}), ("N 0", {"N": 0}), ("K 0", {"K": 0})]),
    "crnn_gemm_f32x3_bnstats": (
        _BN3, "crnn_gemm_f32x3_bnstats_supported", ["M", "N", "K"], [dict(M=958464, N=64, K=128), dict(M=239616, N=256, K=512)],
        [("M % 128", {"M": ("+", 64)}), ("N 96", {"N": 96}), ("N 192", {"N": 192}), ("K % 64", {"K": ("+", 32)}), ("M 2^31", {"M": 1 << 31}), ("M 0", {"M": 0})],
        [("N 0", {"N": 0}), ("K 0", {"K": 0})]),
    "crnn_gemm_f32x2_bnstats": (
        _BN3, "crnn_gemm_f32x3_bnstats_supported", ["M", "N", "K"], [dict(M=958464, N=64, K=128), dict(M=239616, N=256, K=512)],
        [("M % 128", {"M": ("+", 64)}), ("N 96", {"N": 96}), ("N 192", {"N": 192}), ("K % 64", {"K": ("+", 32)}), ("M 2^31", {"M": 1 << 31}), ("M 0", {"M": 0})],
        [("N 0", {"N": 0}), ("K 0", {"K": 0})]),
    "crnn_rnn_input_proj": (
        [("X", "A"), ("Wf", "A"), ("Wb", "A"), ("bias_f", "a"), ("bias_b", "a"), ("Yf", "A"), ("Yb", "A")] + [(n, None) for n in _NT_SHAPE], "crnn_rnn_input_proj_supported_ld", _NT_SHAPE,
        [dict(M=TB, N=G, K=128, lda=128, ldw=128, ldy=G), dict(M=TB, N=G, K=256, lda=256, ldw=256, ldy=G)],
        [("M % 64", {"M": ("+", 32)}), ("N % 256", {"N": ("+", 128), "ldy": ("+", 128)}), ("K 320", {"K": 320, "lda": 320, "ldw": 320}), ("K 96", {"K": 96}),
         ("small model", dict(M=88, N=256, K=32, lda=32, ldw=32, ldy=256)), ("row offsets", {"M": 1 << 21})] + _ld_rules(["lda<K", "ldw<K", "ldy<N"], 8),
        [("one bias", {"bias_b": None, "bias_f": 0x7e0000000000})]),
    "crnn_dense_fwd_stream": (
        [("X", "A"), ("WT", "A"), ("bias", "a"), ("Y", "A"), ("M", None), ("N", None), ("K", None), ("lda", None), ("ldw", None), ("relu", None), ("permP", None), ("drop_rate", None),
         ("seed", None), ("layer", None)], "crnn_dense_fwd_stream_supported_ld", ["M", "N", "K", "lda", "ldw", "permP"],
        [dict(M=TB, N=128, K=FEAT, lda=FEAT, ldw=FEAT, permP=52), dict(M=TB, N=256, K=FEAT, lda=FEAT, ldw=FEAT, permP=0)],
        [("M % 64", {"M": ("+", 32)}), ("N 192", {"N": 192}), ("K % 64", {"K": ("+", 32), "lda": ("+", 32), "ldw": ("+", 32)}), ("permP 5", {"permP": 5}),
         ("small model", dict(M=88, N=32, K=FEAT, lda=FEAT, ldw=FEAT, permP=22)), ("row offsets", {"M": 1 << 19})] + _ld_rules(["lda<K", "ldw<K"], 8),
        [("permP -1", {"permP": -1}), ("rate 1", {"drop_rate": 1.0}), ("rate < 0", {"drop_rate": -0.5})]),
    "crnn_gemm_nt_f32_stream_bias": (
        _NT + [("bias", "a")] + [(n, None) for n in _NT_SHAPE], "crnn_gemm_nt_f32_stream_bias_supported", _NT_SHAPE,
        [dict(M=TB, N=128, K=512, lda=512, ldw=512, ldy=128), dict(M=TB, N=G, K=128, lda=128, ldw=128, ldy=G)],
        [("M % 64", {"M": ("+", 32)}), ("N % 128", {"N": ("+", 64), "ldy": ("+", 64)}), ("K % 64", {"K": ("+", 32), "lda": ("+", 32), "ldw": ("+", 32)}),
         ("small model", dict(M=88, N=256, K=32, lda=32, ldw=32, ldy=256)), ("row offsets", {"M": 1 << 22})] + _ld_rules(["lda<K", "ldw<K", "ldy<N"], 8),
        [("M 0", {"M": 0}), ("N 0", {"N": 0}), ("K 0", {"K": 0}), ("A1 without W1", {"A1": 0x7e0000000000})]),
    "crnn_gemm_nt_f32_stream": (
        _NT + [(n, None) for n in _NT_SHAPE], "crnn_gemm_nt_f32_stream_supported", _NT_SHAPE,
        [dict(M=TB, N=256, K=G, lda=G, ldw=G, ldy=256), dict(M=TB, N=128, K=G, lda=G, ldw=G, ldy=128)],
        [("M % 64", {"M": ("+", 32)}), ("N 384", {"N": 384, "ldy": 384}), ("N 0", {"N": 0}), ("K % 64", {"K": ("+", 32), "lda": ("+", 32), "ldw": ("+", 32)}),
         ("small model", dict(M=88, N=32, K=256, lda=256, ldw=256, ldy=32)), ("row offsets", {"M": 1 << 21})] + _ld_rules(["lda<K", "ldw<K", "ldy<N"], 8),
        [("M 0", {"M": 0}), ("K 0", {"K": 0}), ("A1 without W1", {"A1": 0x7e0000000000})]),
    "crnn_gemm_nt_f32x2_stream": (
        _NT + [(n, None) for n in _NT_SHAPE], "crnn_gemm_nt_f32x2_stream_supported", _NT_SHAPE,
        [dict(M=TB, N=256, K=G, lda=G, ldw=G, ldy=256), dict(M=TB, N=128, K=G, lda=G, ldw=G, ldy=128)],
        [("M % 64", {"M": ("+", 32)}), ("N % 128", {"N": ("+", 64), "ldy": ("+", 64)}), ("K % 64", {"K": ("+", 32), "lda": ("+", 32), "ldw": ("+", 32)}),
         ("small model", dict(M=88, N=32, K=256, lda=256, ldw=256, ldy=32)), ("row offsets", {"M": 1 << 21})] + _ld_rules(["lda<K", "ldw<K", "ldy<N"], 4),
        [("M 0", {"M": 0}), ("N 0", {"N": 0}), ("K 0", {"K": 0}), ("A1 without W1", {"A1": 0x7e0000000000})]),
    "crnn_gemm_tn_stream": (
        _TN("U"), "crnn_gemm_tn_stream_supported", _TN_SHAPE,
        [dict(M=128, N=G, K=TB, lda=128, ldb=G, ldc=G, scratch_bytes=MiB64), dict(M=256, N=G, K=TB - 256, lda=512, ldb=G, ldc=G, scratch_bytes=MiB64)],
        [("M % 128", {"M": ("+", 64), "lda": ("+", 64)}), ("N % 128", {"N": ("+", 64), "ldb": ("+", 64), "ldc": ("+", 64)}), ("N 1152", {"N": 1152, "ldb": 1152, "ldc": 1152}),
         ("K % 64", {"K": ("+", 32)}), ("small model", dict(M=64, N=256, K=88, lda=64, ldb=256, ldc=256)), ("row offsets", {"K": 1 << 20}), ("scratch 1 KiB", {"scratch_bytes": 1024}),
         ("scratch one byte short", {"scratch_bytes": "short"})] + _ld_rules(["lda<M", "ldb<N", "ldc<N"], 4), []),
    "crnn_gemm_tn_planes_stream": (
        _TN("A"), "crnn_gemm_tn_planes_stream_supported", _TN_SHAPE,
        [dict(M=128, N=G, K=TB, lda=128, ldb=G, ldc=G, scratch_bytes=MiB64), dict(M=256, N=G, K=TB - 256, lda=512, ldb=G, ldc=G, scratch_bytes=MiB64),
         dict(M=FEAT, N=128, K=TB, lda=FEAT, ldb=128, ldc=128, scratch_bytes=MiB64)],
        [("M % 128", {"M": ("+", 64), "lda": ("+", 64)}), ("N % 128", {"N": ("+", 64), "ldb": ("+", 64), "ldc": ("+", 64)}), ("K % 32", {"K": ("+", 16)}),
         ("small model", dict(M=64, N=256, K=88, lda=64, ldb=256, ldc=256)), ("row offsets", {"K": 1 << 21}), ("scratch 1 KiB", {"scratch_bytes": 1024}),
         ("scratch one byte short", {"scratch_bytes": "short"})] + _ld_rules(["lda<M", "ldb<N", "ldc<N"], 4), []),
    "crnn_gemm_tn_bf16_stream": (
        _TN("A"), "crnn_gemm_tn_bf16_stream_supported_ld", _TN_SHAPE, [dict(M=FEAT, N=128, K=TB, lda=FEAT, ldb=128, ldc=128, scratch_bytes=MiB64)],
        [("M % 128", {"M": ("+", 64), "lda": ("+", 64)}), ("M 9216", {"M": 9216, "lda": 9216}), ("N % 128", {"N": ("+", 64), "ldb": ("+", 64), "ldc": ("+", 64)}), ("K % 64", {"K": ("+", 32)}),
         ("small model", dict(M=FEAT, N=32, K=88, lda=FEAT, ldb=32, ldc=32)), ("row offsets", {"K": 1 << 18, "lda": 8192}), ("scratch 1 KiB", {"scratch_bytes": 1024}),
         ("scratch one byte short", {"scratch_bytes": "short"}), ("ldc % 4", {"ldc": ("+", 2)})] + _ld_rules(["lda<M", "ldb<N"], 8) + [("ldc short", {"ldc": ("below", "N", 4)})], []),
    "crnn_dropout_keep": (
        [("x", "A"), ("y", "A"), ("keep", "R"), ("rows", None), ("C", None), ("ldx", None), ("ldy", None), ("rate", None), ("seed", None), ("layer", None)], "crnn_dropout_keep_supported",
        ["rows", "C", "ldx", "ldy"], [dict(rows=TB, C=512, ldx=512, ldy=512), dict(rows=88, C=128, ldx=128, ldy=128)],
        [("C % 8", {"C": ("+", 4)}), ("ldx % 4", {"ldx": ("+", 2)}), ("ldy % 4", {"ldy": ("+", 2)}), ("rows 0", {"rows": 0}), ("group counter", {"rows": 1 << 28})], [("rate 1", {"rate": 1.0})]),
}
# what the size queries of the recorded revision answer for a reduction over K rows into [M][N]: the scratch the "one byte short" patterns miss by one
SCRATCH = {"crnn_gemm_tn_stream": lambda L, s: L.crnn_pwconv_wgrad_stream_scratch_bytes(s["K"], s["N"], s["M"]),
           "crnn_gemm_tn_planes_stream": lambda L, s: L.crnn_pwconv_wgrad_planes_stream_scratch_bytes(s["K"], s["N"], s["M"]),
           "crnn_gemm_tn_bf16_stream": lambda L, s: L.crnn_gemm_tn_bf16_stream_scratch_bytes(s["M"], s["N"], s["K"])}
DEFAULTS = dict(relu=1, drop_rate=0.4, rate=0.2, seed=7, layer=9)


def load(path):
    """The library at `path` with the header's argument types for the functions it has (no torch: nothing here touches a device)."""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(here)), "crnn-ocr-lite_amd"))
    from crnn_mi355x import native
    L = ctypes.CDLL(path)
    for name, (ret, args) in native.parse_header().items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ret, args
    return L


def patterns(L):
    """-> [(key, launcher, kind, {argument: value})], kind = null | align | rule | arg; the library only answers the scratch-size queries"""
    out = []
    for fn, (sig, _, _, accepted, rules, arg_errors) in LAUNCHERS.items():
        for si, shape in enumerate(accepted):
            base = dict(DEFAULTS)
            for i, (n, kind) in enumerate(sig):
                if kind in ("A", "U", "R"):
                    base[n] = 0x7f0000000000 + 0x1000000 * (i + 1)      # 16-byte aligned, never dereferenced
                elif kind == "a":
                    base[n] = None
            base.update(shape)

            def add(kind, what, change):
                args = dict(base)
                for n, v in change.items():
                    if v == "short":
                        v = SCRATCH[fn](L, args) - 1
                    args[n] = v if not isinstance(v, tuple) else base[n] + v[1] if v[0] == "+" else base[v[1]] - v[2]
                out.append(("%s set%d %s: %s" % (fn, si, kind, what), fn, kind, args))
            for n, kind in sig:
                if kind in ("A", "R"):
                    add("null", n, {n: None})
                if kind in ("A", "U"):
                    add("align", n, {n: base[n] + 4})
                if kind == "a":
                    pair = {"A1": "W1", "W1": "A1", "bias_f": "bias_b", "bias_b": "bias_f"}.get(n)     # (operands that come in pairs: both present)
                    add("align", n, dict({n: 0x7e0000000000 + 4}, **({pair: 0x7e0001000000} if pair else {})))
            for what, change in rules:
                add("rule", what, change)
            for what, change in arg_errors:
                add("arg", what, change)
    return out


def call(L, fn, args):
    return getattr(L, fn)(*([args[n] for n, _ in LAUNCHERS[fn][0]] + [None]))     # (+ the stream)


def query(L, fn, args):
    return getattr(L, LAUNCHERS[fn][1])(*[args[n] for n in LAUNCHERS[fn][2]])


def records(L):
    """-> {pattern key: return code}"""
    return {key: call(L, fn, args) for key, fn, _, args in patterns(L)}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("-o", "--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_gemm_refusals.json"))
    a = ap.parse_args()
    rec = records(load(a.lib))
    assert all(v in (-2, -3) for v in rec.values()), "a pattern was not refused: %s" % [k for k, v in rec.items() if v not in (-2, -3)]
    json.dump({"records": rec}, open(a.out, "w"), indent=0, sort_keys=True)
    print("%d patterns -> %s" % (len(rec), a.out))
