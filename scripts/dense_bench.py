#!/usr/bin/env python3
"""dense2's one-pass backward (crnn_dense_bwd_small, dense.hip) at the headline shape (M = 52 * B rows, K = 512, C = 38): the product library and any
variant builds of dense.hip found as scripts/_trace/libdense_*.so, each timed over cold tensors (the row tensors rotate over 16 copies).  The ablation
and trace builds this once read are gone; their figures are in profiles/r05_dense_bwd_bench.txt."""
import ctypes, glob, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np
import torch
from crnn_mi355x import native
P = lambda t: ctypes.c_void_p(t.data_ptr())
S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
M, K, C = 52 * B, 512, 38
L0 = native.lib()
nb = L0.crnn_dense_bwd_small_scratch_bytes(M, K, C)
NR = 16
xs = [torch.randn(M, K, device="cuda") for _ in range(NR)]; dxs = [torch.empty(M, K, device="cuda") for _ in range(NR)]
dy = torch.randn(M, C, device="cuda") * 0.1; W = torch.randn(K, C, device="cuda"); g = torch.zeros(K * C + C, device="cuda"); scr = torch.empty(nb // 4, device="cuda")
keep = torch.zeros(M * K // 8 + 4, dtype=torch.uint8, device="cuda"); L0.crnn_dropout_keep_bytes(P(keep), M * K // 8, 0.2, 77, 9, S())
variants = [("product", L0)] + [(os.path.basename(p)[8:-3], ctypes.CDLL(p)) for p in sorted(glob.glob(os.path.join(ROOT, "scripts/_trace/libdense_*.so")))]
for name, L in variants:
    fn = L.crnn_dense_bwd_small
    fn.argtypes = L0.crnn_dense_bwd_small.argtypes; fn.restype = ctypes.c_int
    ms = []
    for it in range(NR + 4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        i = it % NR
        e0.record()
        rc = fn(P(xs[i]), P(dy), P(W), P(dxs[i]), P(g), P(g[K * C:]), P(scr), nb, M, K, C, K, K, P(keep), 0.2, 77, 9, S())
        e1.record(); torch.cuda.synchronize()
        assert rc == 0, rc
        if it >= 4: ms.append(e0.elapsed_time(e1))
    print("%-10s %.1f us (median of %d, kernel + second-stage sum, incl. ~2 us of event latency); %d MB of row tensors" % (name, 1e3 * np.median(ms), NR, 2 * M * K * 4 / 1e6 + M * C * 4 / 1e6), flush=True)
