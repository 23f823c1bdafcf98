#!/usr/bin/env python3
"""Record the workspace plan and the block-output fusion answers of the built library: tests/golden/workspace_plan.json.

Host arithmetic only (crnn_workspace_bytes, crnn_ws_tensor_info, crnn_block_output_fused): runs without a GPU; the device-count queries
behind the partial-row counts fall back to the MI355X's 256 CUs.  Run it from the commit whose plan is to be pinned:
    python tests/golden/make_workspace_plan.py
tests/test_host_cpu.py recomputes records() from the library under test and compares for equality."""
import ctypes
import itertools
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "workspace_plan.json")

# (batch, imgh, imgw, classes, max_len, tds, units)
SHAPES = [(4, 100, 32, 38, 23, 128, 256), (5, 60, 48, 20, 10, 64, 128), (3, 40, 32, 38, 6, 32, 64), (3, 40, 64, 38, 6, 32, 128),
          (3, 200, 32, 62, 21, 128, 256), (64, 100, 32, 38, 23, 128, 256), (256, 100, 32, 38, 23, 128, 256)]
COMBOS = [2 | 32, 2 | 32 | 8, 2 | 32 | 1, 2 | 32 | 16, 1024 | 2048, 4096 | 16, 4096 | 16 | 32]
# tensors whose presence or size is a schedule decision, then every per-block family, then the tensors behind the last of them
NAMES = (["bn2parts", "gbm16", "locterms", "d2part", "keep9", "rnnx", "pwT", "partials", "lg128", "gA", "pbf", "partials2"] +
         [f + str(i) for i in range(1, 8) for f in ("bn1s", "bn2s", "d", "a", "q", "x", "qm", "dm")])


def flag_values(native):
    single = sorted(v for k, v in vars(native).items() if k.startswith("FLAG_"))
    return [0] + single + COMBOS


def configs(native):
    """(key, crnn_config) in a fixed order: shapes x cell x stn x precision mode x flags"""
    for (shape, gru, stn, mode, flags) in itertools.product(SHAPES, (0, 1), (1, 0), (0, 1, 2), flag_values(native)):
        B, h, w, C, L, tds, u = shape
        yield ("%dx%dx%d c%d l%d t%d u%d gru%d stn%d m%d f%d" % (B, h, w, C, L, tds, u, gru, stn, mode, flags),
               native.crnn_config(B, h, w, C, L, tds, u, gru, stn, 1, mode, flags))


def records(native):
    """One [workspace bytes, block-output-fused bit mask (bit i-1 = block i), CRC-32 of the (name, offset, count, dtype | absent) list] per
    configuration, in the order of configs()"""
    L = ctypes.CDLL(native.LIB_PATH)
    L.crnn_workspace_bytes.restype = ctypes.c_size_t
    off, cnt, dt = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    names = [n.encode() for n in NAMES]
    out = []
    for key, cfg in configs(native):
        c = ctypes.byref(cfg)
        fused = sum(1 << (i - 1) for i in range(1, 8) if L.crnn_block_output_fused(c, i))
        rows = []
        for n in names:
            if L.crnn_ws_tensor_info(c, n, ctypes.byref(off), ctypes.byref(cnt), ctypes.byref(dt)) == 0:
                rows.append("%s %d %d %d" % (n.decode(), off.value, cnt.value, dt.value))
            else:
                rows.append("%s absent" % n.decode())
        out.append([int(L.crnn_workspace_bytes(c)), fused, zlib.crc32("\n".join(rows).encode())])
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "crnn-ocr-lite_amd"))
    from crnn_mi355x import native
    rec = records(native)
    with open(OUT, "w") as f:
        json.dump({"shapes": SHAPES, "flags": flag_values(native), "names": NAMES, "records": rec}, f, separators=(",", ":"))
    print("wrote", OUT, len(rec), "configurations")
