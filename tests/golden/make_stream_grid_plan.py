#!/usr/bin/env python3
"""Record what the streamed pointwise GEMMs' host plans answer: tests/golden/stream_grid_plan.json.

Host arithmetic only (the *_supported, *_rows / *_stat_rows and *_scratch_bytes entry points of gemm_wres, gemm_wres3, gemm_pres, gemm_wgrad and
gemm_wgrad3): runs without a GPU; the CU-count query behind the grids falls back to the MI355X's 256 CUs.  The grid size itself is not exported;
the partial-statistics rows (stripe grid) and the scratch bytes (reduction-split grid) are functions of it.  Run it from the commit whose plans
are to be pinned:
    python tests/golden/make_stream_grid_plan.py
tests/test_host_cpu.py recomputes records() from the library under test and compares for equality."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "stream_grid_plan.json")

# pixels of the CRNN's blocks (104 x 36 before block 3's pooling, 52 x 18 before block 5's, 52 x 9 after) at batch 8 and at batch 256; dense1's
# T * B rows at batch 256; 40 and 8 stripes of 128 (fewer than 8 XCDs x Q lanes); a single stripe / chunk of each kernel; a ragged M (refused)
MS = [8 * 3744, 8 * 936, 8 * 468, 256 * 3744, 256 * 936, 256 * 468, 13312, 5120, 1024, 128, 64, 32, 100]
CH = [64, 128, 256, 512]
# (N, K): the pointwise shapes, then channel counts every kernel refuses
NK = [(n, k) for n in CH for k in CH] + [(96, 256), (128, 192), (2048, 256)]
# dense1 (4608 features = 36 tiles of 128: more tiles than an XCD has CUs) as (M, N, K) of the C[M][N] = A^T . B calls, and a refused one
TN = [(4608, 128, 13312), (4608, 128, 3328), (4608, 256, 64), (4600, 128, 13312)]

LONG, INT, SIZE = ctypes.c_long, ctypes.c_int, ctypes.c_size_t
# name -> (restype, argtypes); called with (M, N, K) unless noted in records()
CALLS = {
    "crnn_gemm_wres_supported": (INT, [INT, INT]),
    "crnn_gemm_wres_bnstats_supported": (INT, [LONG, INT, INT]),
    "crnn_gemm_wres_bnstats_rows": (INT, [LONG, INT, INT]),
    "crnn_pwconv_fwd_wres_supported": (INT, [LONG, INT, INT]),
    "crnn_pwconv_fwd_wres_rows": (INT, [LONG, INT, INT]),
    "crnn_gemm_wres3_supported": (INT, [LONG, INT, INT]),
    "crnn_gemm_wres3_stat_rows": (INT, [LONG, INT, INT]),
    "crnn_gemm_pres_supported": (INT, [LONG, INT, INT, INT]),
    "crnn_gemm_pres_stat_rows": (INT, [LONG, INT, INT, INT]),
    "crnn_pwconv_wgrad_stream_scratch_bytes": (SIZE, [LONG, INT, INT]),
    "crnn_pwconv_wgrad_planes_stream_scratch_bytes": (SIZE, [LONG, INT, INT]),
    "crnn_gemm_tn_bf16_stream_scratch_bytes": (SIZE, [INT, INT, LONG]),
}


def records(lib_path):
    """{key: value} in a fixed order: every call of CALLS over MS x NK (pres: two and three planes), then the dense1 shapes"""
    L = ctypes.CDLL(lib_path)
    for name, (res, args) in CALLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    out = {}
    for n, k in NK:
        out["wres_supported N%d K%d" % (n, k)] = L.crnn_gemm_wres_supported(n, k)
    for m in MS:
        for n, k in NK:
            key = "M%d N%d K%d" % (m, n, k)
            for name in ("crnn_gemm_wres_bnstats_supported", "crnn_gemm_wres_bnstats_rows", "crnn_pwconv_fwd_wres_supported", "crnn_pwconv_fwd_wres_rows",
                         "crnn_gemm_wres3_supported", "crnn_gemm_wres3_stat_rows", "crnn_pwconv_wgrad_stream_scratch_bytes",
                         "crnn_pwconv_wgrad_planes_stream_scratch_bytes"):
                out["%s %s" % (name[5:], key)] = int(getattr(L, name)(m, n, k))
            for planes in (2, 3):
                out["gemm_pres_supported p%d %s" % (planes, key)] = L.crnn_gemm_pres_supported(m, n, k, planes)
                out["gemm_pres_stat_rows p%d %s" % (planes, key)] = L.crnn_gemm_pres_stat_rows(m, n, k, planes)
    for m, n, k in TN:
        out["gemm_tn_bf16_stream_scratch_bytes M%d N%d K%d" % (m, n, k)] = int(L.crnn_gemm_tn_bf16_stream_scratch_bytes(m, n, k))
        # the planes stream takes the same product as (pixels = k, channels out = n, channels in = m)
        out["pwconv_wgrad_planes_stream_scratch_bytes M%d N%d K%d" % (k, n, m)] = int(L.crnn_pwconv_wgrad_planes_stream_scratch_bytes(k, n, m))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "crnn-ocr-lite_amd"))
    from crnn_mi355x import native
    rec = records(native.LIB_PATH)
    with open(OUT, "w") as f:
        json.dump({"ms": MS, "nk": [list(s) for s in NK], "tn": [list(s) for s in TN], "records": rec}, f, separators=(",", ":"))
    print("wrote", OUT, len(rec), "values")
