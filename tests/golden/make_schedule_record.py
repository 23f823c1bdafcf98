#!/usr/bin/env python3
"""Record what crnn_schedule_describe answers: tests/golden/schedule_record.json.

The step driver's schedule record as text, over the configurations of make_workspace_plan.py (shapes x LSTM / GRU x stn x precision mode x flags) times the
alignment masks 7 (every base pointer 16-byte aligned), 6 (workspace not), 5 (parameters not), 3 (gradients not) and 0.  Host arithmetic only: runs without a
GPU.  Run it from the commit whose record is to be pinned:
    python tests/golden/make_schedule_record.py
The file holds one CRC-32 of the text per configuration and mask, and the whole text for the benchmarked shape (batch 256, 100x32, LSTM, stn) in the three
precision modes with every pointer aligned.  It is a change detector: tests/test_host_cpu.py recomputes records() from the library under test and compares."""
import ctypes
import importlib.util
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "schedule_record.json")
MASKS = [7, 6, 5, 3, 0]
BENCH = "256x100x32 c38 l23 t128 u256 gru0 stn1 m%d f0"     # (keys of make_workspace_plan.configs)


def plan_module():
    spec = importlib.util.spec_from_file_location("make_workspace_plan", os.path.join(HERE, "make_workspace_plan.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def describe(L, cfg, mask):
    """The text for one configuration and alignment mask (asked for its length first)"""
    n = L.crnn_schedule_describe(ctypes.byref(cfg), mask, None, 0)
    assert n > 0, n
    buf = ctypes.create_string_buffer(n + 1)
    assert L.crnn_schedule_describe(ctypes.byref(cfg), mask, buf, n + 1) == n
    return buf.value.decode()


def records(native):
    """-> ([[CRC-32 per mask] per configuration, in the order of make_workspace_plan.configs()], {benchmarked key: text at mask 7})"""
    L = ctypes.CDLL(native.LIB_PATH)
    L.crnn_schedule_describe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    crcs, texts = [], {}
    for key, cfg in plan_module().configs(native):
        crcs.append([zlib.crc32(describe(L, cfg, m).encode()) for m in MASKS])
        if key in [BENCH % m for m in (0, 1, 2)]:
            texts[key] = describe(L, cfg, 7).split("\n")
    return crcs, texts


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "crnn-ocr-lite_amd"))
    from crnn_mi355x import native
    crcs, texts = records(native)
    with open(OUT, "w") as f:
        json.dump({"masks": MASKS, "records": crcs, "benchmarked": texts}, f, separators=(",", ":"))
    print("wrote", OUT, len(crcs), "configurations x", len(MASKS), "masks")
