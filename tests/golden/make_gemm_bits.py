#!/usr/bin/env python3
"""Record the output bits of the tile GEMM entry points of the built library: tests/golden/gemm_bits.npz.

The tile GEMM (csrc/gemm.hip, gemm_bf16.hip, gemm_planes.hip) is the fallback of every resident / streaming GEMM and the reference the
`*_equals_the_tile_kernel` tests hold the faster kernels against, so a mistake in it moves both sides of those tests; this pins its results
from outside.  cases() reaches every launch branch of the host planner at the smallest shape that takes it: the fp32, bf16 and plane kernels
in the three operand modes at both tile widths, whole and guarded tiles, vector-legal and unaligned operands, every epilogue, the producer
prologues, the split reductions with each second stage, and the calls that must be refused without a store.  Outputs only: the inputs are
rebuilt from seeds (numpy's frozen RandomState), with a few denormal, negative-zero and large entries and no NaN / Inf.  Small outputs are
stored whole as int32 bit patterns, larger ones as the sha256 of their bytes plus their first 16 words.  Needs the MI355X; run it from the
commit whose bits are to be pinned:
    python tests/golden/make_gemm_bits.py
tests/test_gpu_gemm_bits.py recomputes arrays() with the library under test and compares.  The fixture holds for the compiler it was
recorded with: `hipcc --version` is stored beside the arrays."""
import hashlib
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gemm_bits.npz")
MAX_BYTES = 300 * 1000
WHOLE_MAX = 260                        # outputs of up to this many words are stored whole
F32, BF16 = 0, 1
SENTINEL = 7.0                         # every output buffer starts as this (fp32 0x40e00000, bf16 0x40e0)
ERR_ARG, ERR_UNSUPPORTED = -2, -3

WHOLE = ((128, 128, 64), (128, 64, 64))                                  # (M, N, K): whole tiles at both tile widths, 16-byte accesses legal
GUARDED = ((77, 20, 25), (300, 130, 70), (260, 1, 64),                  # partial tiles, scalar accesses
           (200, 72, 96), (136, 40, 64))                                 # partial tiles, 16-byte accesses legal for fp32 and bf16 storage
F32_SHAPES = ((128, 64, 32), (128, 128, 64), (77, 20, 25), (300, 130, 70), (200, 72, 96))


def hipcc_version():
    try:
        return subprocess.run(["hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout.strip()
    except OSError as e:
        return "hipcc --version: %s" % e


def bits(a):
    """float32 -> its int32 bit patterns (the sign of zero and denormals included); 16-bit words (bf16) widened; other integers as int32"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.int32)
    if a.dtype in (np.int16, np.uint16):
        return a.view(np.uint16).astype(np.int32)
    return a.astype(np.int32)


def summary(a):
    """what the fixture keeps of one output: a small array whole, a larger one as (sha256 of its little-endian words, its first 16 words)"""
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    if a.size <= WHOLE_MAX:
        return a
    return np.frombuffer(hashlib.sha256(a.astype("<i4").tobytes()).digest(), dtype=np.uint8).copy(), a[:16].copy()


def stored(rec):
    """{name: int32 array} -> the fixture's few packed arrays (one archive member per output would cost more than the outputs)"""
    names = sorted(rec)
    whole, sha, head = [np.zeros(0, np.int32)], [np.zeros((0, 32), np.uint8)], [np.zeros((0, 16), np.int32)]
    for n in names:
        s = summary(rec[n])
        if isinstance(s, tuple):
            sha.append(s[0][None]); head.append(s[1][None])
        else:
            whole.append(s)
    return {"names": np.array(names), "sizes": np.array([rec[n].size for n in names], dtype=np.int64), "whole": np.concatenate(whole),
            "sha256": np.concatenate(sha), "head": np.concatenate(head)}


def unpack(packed):
    """stored()'s arrays -> {name: summary()}"""
    out, w, d = {}, 0, 0
    for n, size in zip(packed["names"].tolist(), packed["sizes"].tolist()):
        if size <= WHOLE_MAX:
            out[n] = packed["whole"][w:w + size]; w += size
        else:
            out[n] = (packed["sha256"][d], packed["head"][d]); d += 1
    assert w == packed["whole"].size and d == len(packed["sha256"])
    return out


def load(path=OUT):
    """-> ({name: summary()} of every recorded output, the recorded `hipcc --version`)"""
    gold = np.load(path)
    return unpack({k: gold[k] for k in gold.files if k != "hipcc_version"}), str(gold["hipcc_version"])


def same(a, b):
    """two summary() values are equal"""
    if isinstance(a, tuple) != isinstance(b, tuple):
        return False
    return all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def values(name, shape, special=True):
    """seeded N(0, 1) fp32 values; `special`: two denormals, a negative zero and two large entries at fixed places"""
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    a = rs.standard_normal(size=shape).astype(np.float32)
    f = a.reshape(-1)
    n = f.size
    if special and n >= 8:
        f[1] = np.float32(1e-40); f[n - 2] = np.float32(-1e-41)
        f[n // 3] = np.float32(-0.0)
        f[n // 2] = np.float32(2.0 ** 20); f[2 * n // 3] = np.float32(-2.0 ** 18)
    return a


def bnstate(name, n):
    """[mean | var | scale | shift] x n of a BatchNorm (var > 0)"""
    s = values(name, (4, n), special=False)
    s[1] = np.abs(s[1]) + 0.5
    return s


def to_bf16(a):
    """fp32 -> bf16 words, round to nearest even (finite values)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7fff)) >> 16).astype(np.uint16)


class _Run:
    """one case on the device: operands in, sentinel-filled outputs, results back as bits"""

    def __init__(self):
        import torch
        import gpu_util
        self.torch, self.g = torch, gpu_util
        self.L = gpu_util.L()

    def dev(self, a, dt=F32):
        t = self.torch.from_numpy(to_bf16(a).view(np.int16) if dt == BF16 else np.ascontiguousarray(a, dtype=np.float32)).cuda()
        self.g._KEEP.append(t)
        return t

    def fill(self, shape, dt=F32):
        t = self.torch.full(shape, 0x40e0, dtype=self.torch.int16, device="cuda") if dt == BF16 else self.torch.full(shape, SENTINEL, device="cuda")
        self.g._KEEP.append(t)
        return t

    def done(self, out, name, code, **tensors):
        self.torch.cuda.synchronize()
        out[name + " code"] = np.array([code], dtype=np.int32)
        for k, t in tensors.items():
            if t is not None:
                out["%s %s" % (name, k)] = bits(self.g.host(t))
        self.g.release()


def _gemm(r, out, name, entry, mode, M, N, K, dt=(F32, F32, F32), bias=0, act=0, acc=0, perm=0, scratch=0, pad=0):
    """crnn_gemm_f32 | crnn_gemm_bf16_ex | crnn_gemm_f32x3 | crnn_gemm_f32x2; `scratch` in floats, `pad` elements on every leading dimension"""
    P, S = r.g.P, r.g.S
    a_shape = (K, M + pad) if mode == 2 else (M, K + pad)
    b_shape = (N, K + pad) if mode == 1 else (K, N + pad)
    A, B = r.dev(values(name + " A", a_shape), dt[0]), r.dev(values(name + " B", b_shape), dt[1])
    C = r.dev(values(name + " C", (M, N + pad)), dt[2]) if acc else r.fill((M, N + pad), dt[2])
    bv = r.dev(values(name + " bias", (N,))) if bias else None
    scr = r.fill((scratch,)) if scratch else None
    args = (mode, P(A), P(B), P(C), M, N, K, a_shape[1], b_shape[1], N + pad, P(bv), act, acc, perm, P(scr), scratch * 4)
    if entry == "bf16":
        code = r.L.crnn_gemm_bf16_ex(*args, dt[0], dt[1], dt[2], S())
    else:
        code = getattr(r.L, "crnn_gemm_" + entry)(*args, S())
    r.done(out, name, code, C=C)


def _pwconv(r, out, name, M, N, K, products, dt=(F32, F32, F32), wt=0, stats=False, fold=False):
    """crnn_pwconv_fwd: products 0 fp32 MFMA, 1 bf16, 2 three planes, 3 two planes"""
    P, S = r.g.P, r.g.S
    a, w = r.dev(values(name + " a", (M, K)), dt[0]), r.dev(values(name + " w", (N, K) if wt else (K, N)), dt[1])
    q = r.fill((M, N), dt[2])
    part = r.fill((r.L.crnn_pwconv_stat_rows(M), 2, N)) if stats else None
    st = r.dev(bnstate(name + " bn", N)) if fold else None
    code = r.L.crnn_pwconv_fwd(P(a), P(w), P(q), M, N, K, P(part), P(st), products, dt[0], dt[1], dt[2], wt, S())
    r.done(out, name, code, q=q, stats=part)


def _bn_fwd(r, out, name, kind, M, N, K, dt_q=F32, wt=0, stats=True):
    """crnn_pwconv_bnrelu6_fwd (kind bf16) | _fwd_f32x3 | _fwd_f32x2"""
    P, S = r.g.P, r.g.S
    bf = BF16 if kind == "bf16" else F32
    d, st = r.dev(values(name + " d", (M, K)), bf), r.dev(bnstate(name + " bn", K))
    w = r.dev(values(name + " w", (N, K) if wt else (K, N)), bf)
    q = r.fill((M, N), dt_q)
    part = r.fill((r.L.crnn_pwconv_stat_rows(M), 2, N)) if stats else None
    if kind == "bf16":
        code = r.L.crnn_pwconv_bnrelu6_fwd(P(d), P(st), P(w), P(q), M, N, K, P(part), dt_q, wt, S())
    else:
        code = getattr(r.L, "crnn_pwconv_bnrelu6_fwd_" + kind)(P(d), P(st), P(w), P(q), M, N, K, P(part), S())
    r.done(out, name, code, q=q, stats=part)


def _bn_wgrad(r, out, name, kind, M, N, K, scratch=0):
    """crnn_pwconv_bnrelu6_wgrad (kind bf16) | _wgrad_f32x3 | _wgrad_f32x2: dw [K][N] = ReLU6(BN(d [M][K]))^T . g [M][N]"""
    P, S = r.g.P, r.g.S
    bf = BF16 if kind == "bf16" else F32
    d, st, g = r.dev(values(name + " d", (M, K)), bf), r.dev(bnstate(name + " bn", K)), r.dev(values(name + " g", (M, N)), bf)
    dw = r.fill((K, N))
    scr = r.fill((scratch,)) if scratch else None
    fn = r.L.crnn_pwconv_bnrelu6_wgrad if kind == "bf16" else getattr(r.L, "crnn_pwconv_bnrelu6_wgrad_" + kind)
    code = fn(P(d), P(st), P(g), P(dw), M, N, K, P(scr), scratch * 4, S())
    r.done(out, name, code, dw=dw)


def _bnstats(r, out, name, planes, M, N, K, null=None, offset=None):
    """crnn_gemm_f32x3_bnstats | crnn_gemm_f32x2_bnstats; `null`: that argument is NULL; `offset`: that argument starts 4 bytes into its buffer"""
    import ctypes
    P, S = r.g.P, r.g.S
    t = {"dq": r.dev(values(name + " dq", (M * K + 4,))), "w": r.dev(values(name + " w", (N, K))), "d": r.dev(values(name + " d", (M * N + 4,))),
         "bnstate": r.dev(bnstate(name + " bn", N))}
    da, part = r.fill((M, N)), r.fill((max(M // 128, 1), 2, N))
    ptr = {k: (None if k == null else ctypes.c_void_p(v.data_ptr() + (4 if k == offset else 0))) for k, v in t.items()}
    fn = r.L.crnn_gemm_f32x3_bnstats if planes == 3 else r.L.crnn_gemm_f32x2_bnstats
    code = fn(ptr["dq"], ptr["w"], P(da), M, N, K, ptr["d"], ptr["bnstate"], None if null == "partials" else P(part), S())
    r.done(out, name, code, da=da, stats=part)


def _split3(r, out, name, n, stride):
    P, S = r.g.P, r.g.S
    x = r.dev(values(name + " x", (n,)))
    planes = r.fill((3 * stride,), BF16)
    code = r.L.crnn_split3_planes(P(x), P(planes), n, stride, S())
    r.done(out, name, code, planes=planes)


# ---- the case list -------------------------------------------------------------------------------------------------------------
def cases():
    """[(name, runner, kwargs)]: needs no device, so the list itself can be checked anywhere"""
    c = []

    def add(fn, name, **kw):
        c.append((name, fn, kw))

    def shape(s):
        return "%dx%dx%d" % s

    ENTRIES = (("f32", (F32, F32, F32)), ("bf16", (F32, F32, F32)), ("bf16", (BF16, BF16, BF16)), ("f32x3", (F32, F32, F32)), ("f32x2", (F32, F32, F32)))

    def tag(entry, dt):
        return entry + ("" if entry != "bf16" else " dt%d%d%d" % dt)
    # the three kernels, modes 0/1/2, both tile widths, whole and guarded tiles
    for s in F32_SHAPES:
        for mode in range(3):
            add(_gemm, "f32 mode%d %s" % (mode, shape(s)), entry="f32", mode=mode, M=s[0], N=s[1], K=s[2])
    for s in WHOLE + GUARDED:
        for mode in range(3):
            for dta in (F32, BF16):
                for dtb in (F32, BF16):
                    for dtc in (F32, BF16):
                        add(_gemm, "bf16 dt%d%d%d mode%d %s" % (dta, dtb, dtc, mode, shape(s)), entry="bf16", mode=mode, M=s[0], N=s[1], K=s[2], dt=(dta, dtb, dtc))
            for entry in ("f32x3", "f32x2"):
                add(_gemm, "%s mode%d %s" % (entry, mode, shape(s)), entry=entry, mode=mode, M=s[0], N=s[1], K=s[2])
    # unaligned leading dimensions (vecA / vecB / vecC false on whole-tile shapes) and the epilogue options, per kernel and tile kind
    for entry, dt in ENTRIES:
        for mode in range(3):
            add(_gemm, "%s mode%d 128x128x64 ld+1" % (tag(entry, dt), mode), entry=entry, mode=mode, M=128, N=128, K=64, dt=dt, pad=1)
        for s, P in (((128, 128, 64), 4), ((128, 64, 64), 8), ((300, 130, 70), 3), ((200, 72, 96), 5)):
            opts = (("bias relu", dict(bias=1, act=1)), ("accumulate", dict(acc=1)), ("perm%d" % P, dict(perm=P)),
                    ("bias relu accumulate perm%d" % P, dict(bias=1, act=1, acc=1, perm=P)))
            for oname, o in opts:
                add(_gemm, "%s mode0 %s %s" % (tag(entry, dt), shape(s), oname), entry=entry, mode=0, M=s[0], N=s[1], K=s[2], dt=dt, **o)
        add(_gemm, "%s mode1 128x128x64 bias accumulate ld+4" % tag(entry, dt), entry=entry, mode=1, M=128, N=128, K=64, dt=dt, bias=1, acc=1, pad=4 if dt[0] == F32 else 8)
    # pointwise convolution: statistics epilogue and folded inference BatchNorm, all product kinds
    for products, dts in ((0, ((F32, F32, F32),)), (1, ((F32, F32, F32), (BF16, BF16, BF16), (BF16, BF16, F32))), (2, ((F32, F32, F32),)), (3, ((F32, F32, F32),))):
        for dt in dts:
            for s in ((128, 128, 64), (256, 64, 64), (300, 130, 70), (200, 72, 96), (136, 40, 64)):
                for wt in (0, 1):
                    for what in ("stats", "fold", "plain"):
                        add(_pwconv, "pwconv products%d dt%d%d%d wt%d %s %s" % (products, dt[0], dt[1], dt[2], wt, shape(s), what), M=s[0], N=s[1], K=s[2], products=products,
                            dt=dt, wt=wt, stats=what == "stats", fold=what == "fold")
    # producer prologue, bf16 kernel: modes 0 / 1 (forward) and 2 (weight gradient), whole and guarded, both tile widths
    for s in ((128, 128, 64), (256, 64, 64), (200, 72, 96), (136, 40, 64), (128, 128, 512)):
        for wt in (0, 1):
            for dtq in (F32, BF16):
                add(_bn_fwd, "bnrelu6_fwd bf16 wt%d dtq%d %s" % (wt, dtq, shape(s)), kind="bf16", M=s[0], N=s[1], K=s[2], dt_q=dtq, wt=wt)
    for s in ((64, 128, 128), (128, 64, 256), (100, 72, 136), (72, 40, 64)):
        add(_bn_wgrad, "bnrelu6_wgrad bf16 %s" % shape(s), kind="bf16", M=s[0], N=s[1], K=s[2])
    # ... and the plane kernel's staging prologue, modes 0 and 2, three and two planes (K = 512: the channel table's limit)
    for kind in ("f32x3", "f32x2"):
        for s in ((128, 128, 64), (256, 64, 64), (77, 20, 25), (300, 130, 70), (200, 72, 96), (128, 128, 512)):
            add(_bn_fwd, "bnrelu6_fwd %s %s" % (kind, shape(s)), kind=kind, M=s[0], N=s[1], K=s[2])
        add(_bn_fwd, "bnrelu6_fwd %s 128x64x64 no stats" % kind, kind=kind, M=128, N=64, K=64, stats=False)
        for s in ((64, 128, 128), (128, 64, 256), (100, 72, 136), (77, 20, 25), (70, 130, 300)):
            add(_bn_wgrad, "bnrelu6_wgrad %s %s" % (kind, shape(s)), kind=kind, M=s[0], N=s[1], K=s[2])
    # BatchNorm-backward epilogue of the plane kernel, N = 64 and 128
    for planes in (3, 2):
        for s in ((128, 64, 64), (256, 128, 128)):
            add(_bnstats, "bnstats planes%d %s" % (planes, shape(s)), planes=planes, M=s[0], N=s[1], K=s[2])
    # split reductions (scratch in floats).  M = N = 128: one tile.
    MN = 128 * 128
    for entry, dt in ENTRIES:
        t = tag(entry, dt)
        add(_gemm, "%s split K512 four ranges" % t, entry=entry, mode=2, M=128, N=128, K=512, dt=dt, scratch=4 * MN)                  # 2-D grid, reduce8
        add(_gemm, "%s split K512 scratch for two" % t, entry=entry, mode=2, M=128, N=128, K=512, dt=dt, scratch=2 * MN + 100)       # scratch too small for four
        add(_gemm, "%s split K512 scratch for none" % t, entry=entry, mode=2, M=128, N=128, K=512, dt=dt, scratch=MN - 4)
        add(_gemm, "%s split K1152 sixteen ranges" % t, entry=entry, mode=2, M=128, N=128, K=1152, dt=dt, scratch=16 * MN)             # XCD-pinned, 7 empty ranges
        add(_gemm, "%s split K1152 scratch for nine" % t, entry=entry, mode=2, M=128, N=128, K=1152, dt=dt, scratch=9 * MN)            # 2-D grid, 9 ranges
        add(_gemm, "%s split K16896 more than 32 ranges" % t, entry=entry, mode=2, M=128, N=64, K=16896, dt=dt, scratch=40 * 128 * 64)
        add(_gemm, "%s split K512 guarded 77x20" % t, entry=entry, mode=2, M=77, N=20, K=512, dt=dt, scratch=4 * 77 * 20 + 3)          # (scratch not 16-byte sized)
        add(_gemm, "%s split K512 N130" % t, entry=entry, mode=2, M=100, N=130, K=512, dt=dt, scratch=4 * 100 * 130)                   # N % 4 != 0: the LDS-combining stage
        add(_gemm, "%s split mode0 K2048 bias relu perm accumulate" % t, entry=entry, mode=0, M=128, N=128, K=2048, dt=dt, bias=1, act=1, acc=1, perm=4, scratch=8 * MN)
        add(_gemm, "%s split mode1 K1024 bias" % t, entry=entry, mode=1, M=256, N=64, K=1024, dt=dt, bias=1, scratch=8 * 256 * 64)
        # 17 tiles, K = 512: only the plane products without a bias split
        add(_gemm, "%s 17 tiles K512" % t, entry=entry, mode=2, M=2176, N=64, K=512, dt=dt, scratch=4 * 2176 * 64)
        add(_gemm, "%s 17 tiles K512 bias" % t, entry=entry, mode=2, M=2176, N=64, K=512, dt=dt, bias=1, scratch=4 * 2176 * 64)
    add(_gemm, "bf16 dt001 split K512 four ranges", entry="bf16", mode=2, M=128, N=128, K=512, dt=(F32, F32, BF16), scratch=4 * MN)  # bf16 result of a split
    for kind in ("bf16", "f32x3", "f32x2"):
        add(_bn_wgrad, "bnrelu6_wgrad %s split M1152" % kind, kind=kind, M=1152, N=128, K=128, scratch=16 * MN)
        add(_bn_wgrad, "bnrelu6_wgrad %s split M520 guarded" % kind, kind=kind, M=520, N=72, K=136, scratch=4 * 136 * 72)
    add(_split3, "split3_planes 1024 stride 1028", n=1024, stride=1028)
    add(_split3, "split3_planes 260 stride 260", n=260, stride=260)
    # calls that must be refused before anything is stored
    for entry, dt in ENTRIES:
        t = tag(entry, dt)
        add(_gemm, "refused %s perm does not divide M" % t, entry=entry, mode=0, M=130, N=64, K=64, dt=dt, perm=4)
    add(_pwconv, "refused pwconv fp32 stats with folded BatchNorm", M=128, N=64, K=64, products=0, stats=True, fold=True)
    add(_pwconv, "refused pwconv bf16 stats with folded BatchNorm", M=128, N=64, K=64, products=1, stats=True, fold=True)
    add(_pwconv, "refused pwconv planes stats with folded BatchNorm", M=128, N=64, K=64, products=2, stats=True, fold=True)
    add(_pwconv, "refused pwconv fp32 products of bf16 tensors", M=128, N=64, K=64, products=0, dt=(BF16, BF16, BF16))
    add(_pwconv, "refused pwconv three planes of a bf16 operand", M=128, N=64, K=64, products=2, dt=(BF16, F32, F32))
    add(_pwconv, "refused pwconv two planes of bf16 weights", M=128, N=64, K=64, products=3, dt=(F32, BF16, F32))
    add(_bn_fwd, "refused bnrelu6_fwd bf16 K576", kind="bf16", M=128, N=64, K=576)
    add(_bn_fwd, "refused bnrelu6_fwd bf16 K68 no 16-byte rows", kind="bf16", M=128, N=64, K=68)
    add(_bn_wgrad, "refused bnrelu6_wgrad bf16 K68 no 16-byte rows", kind="bf16", M=128, N=64, K=68)
    add(_bn_fwd, "refused bnrelu6_fwd f32x3 K576", kind="f32x3", M=128, N=64, K=576)
    add(_bn_fwd, "refused bnrelu6_fwd f32x2 K576", kind="f32x2", M=128, N=64, K=576)
    for planes in (3, 2):
        add(_bnstats, "refused bnstats planes%d partial tiles" % planes, planes=planes, M=100, N=64, K=64)
        add(_bnstats, "refused bnstats planes%d N192" % planes, planes=planes, M=128, N=192, K=64)
        for arg in ("d", "bnstate", "partials"):
            add(_bnstats, "refused bnstats planes%d no %s" % (planes, arg), planes=planes, M=128, N=64, K=64, null=arg)
        for arg in ("d", "bnstate", "dq"):
            add(_bnstats, "refused bnstats planes%d %s not 16-byte aligned" % (planes, arg), planes=planes, M=128, N=64, K=64, offset=arg)
    return c


EXPECTED_REFUSALS = {"perm does not divide M": ERR_ARG, "stats with folded BatchNorm": ERR_ARG, "fp32 products of bf16 tensors": ERR_ARG,
                     "planes of a bf16 operand": ERR_ARG, "planes of bf16 weights": ERR_ARG, "K576": ERR_UNSUPPORTED, "no 16-byte rows": ERR_UNSUPPORTED,
                     "partial tiles": ERR_UNSUPPORTED, "N192": ERR_UNSUPPORTED, " no d": ERR_ARG, " no bnstate": ERR_ARG, " no partials": ERR_ARG,
                     "not 16-byte aligned": ERR_UNSUPPORTED}


def arrays():
    """{name: int32 ndarray} of every recorded output and return code, computed with the built library on the current device"""
    r, out = _Run(), {}
    for name, fn, kw in cases():
        fn(r, out, name, **kw)
    return out


def check(rec):
    """what gets pinned has something to pin: accepted calls wrote every element they own, refused ones none, with the return code the header names"""
    sent32, sent16 = int(np.float32(SENTINEL).view(np.int32)), 0x40e0
    for name, _, kw in cases():
        code = int(rec[name + " code"][0])
        outs = {k: a for k, a in rec.items() if k.startswith(name + " ") and not k.endswith(" code") and k[len(name) + 1:] in ("C", "q", "stats", "dw", "da", "planes")}
        assert outs, name
        if name.startswith("refused"):
            want = [v for k, v in EXPECTED_REFUSALS.items() if k in name]
            assert want == [code], (name, code)
            assert all(((a == sent32) | (a == sent16)).all() for a in outs.values()), "%s: a refused call stored something" % name
        else:
            assert code == 0, (name, code)
            for k, a in outs.items():
                own = a[:, :kw["N"]] if k.endswith(" C") and not kw.get("acc") else a
                if k.endswith(" planes"):
                    own = a.reshape(3, -1)[:, :kw["n"]]
                assert not ((own == sent32) | (own == sent16)).all(axis=-1).any(), "%s: rows of %s were not written" % (name, k)
                if k.endswith(" C") and kw.get("pad") and not kw.get("acc"):
                    assert (a[:, kw["N"]:] == (sent16 if kw["dt"][2] == BF16 else sent32)).all(), "%s: the padding of C was written" % name


if __name__ == "__main__":
    tests = os.path.dirname(HERE)
    for p in (os.path.join(os.path.dirname(tests), "crnn-ocr-lite_amd"), tests):
        sys.path.insert(0, p)
    rec = arrays()
    check(rec)
    keep = stored(rec)
    np.savez_compressed(OUT, hipcc_version=np.array(hipcc_version()), **keep)
    size = os.path.getsize(OUT)
    assert size < MAX_BYTES, "%s is %d bytes" % (OUT, size)
    back, _ = load()
    assert sorted(back) == sorted(rec) and all(same(back[k], summary(rec[k])) for k in rec)
    print("wrote", OUT, len(cases()), "cases,", len(rec), "arrays,", len(keep["sha256"]), "as digests,", size, "bytes")
