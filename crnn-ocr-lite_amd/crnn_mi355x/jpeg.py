"""Baseline JPEG decoding: the NumPy definition (`jpeg_decode_host`, `jpeg_gray_host`) and the device path (`JpegDecoder`: crnn_jpeg_plan on the
host, crnn_jpeg_decode in csrc/jpeg.hip) that is held to it bit for bit.  The contract of both is in include/crnn_mi355x.h.

The host definition restates libjpeg's integer pipeline (Huffman decode, dequantisation, jidctint's islow IDCT, "fancy" chroma upsampling, 16-bit
fixed-point YCbCr -> RGB) in int64 arithmetic wrapped to int32 where the library wraps; on files an encoder made from 8-bit pixels it equals
libjpeg-turbo's RGB exactly (tests/test_jpeg_cpu.py).  libjpeg's range-limit table wraps where the clamp here saturates, so the equality is
claimed for encoder-made files only.

GREY.  `data.read_img` forms floor(rgb @ [0.299, 0.587, 0.114] + 0.5) in float64.  At the 16 782 RGB triples where 299 R + 587 G + 114 B + 500
is a multiple of 1000 the exact sum lies on the rounding boundary and NumPy's answer depends on the array's shape (its matmul takes different
summation paths); everywhere else the sum is at least 0.001 from a boundary and every evaluation order agrees.  The rule fixed here, for the
kernel and for `jpeg_gray_host`, is floor(fma(0.114, B, fma(0.587, G, 0.299 R)) + 0.5) with correctly rounded fused multiply-adds -- what
NumPy computes on an (N, 1, 3) array.  So on colour files the device's grey equals read_img's except possibly by 1 at tie pixels (about 0.1 % of
pixels); on greyscale files (R = G = B, never a tie) it equals read_img's everywhere.  `read_img` itself is unchanged.

    dec = JpegDecoder()
    arena, status, shapes = dec.decode(names)           # a pages.PageArena of grey pages; status: device int32, 0 = decoded on the device
"""
import ctypes
import io
from fractions import Fraction

import numpy as np

from . import native
from .pages import PageArena, StagingSlots, device_lib, _ARENA_ALIGN

OK, UNSUPPORTED, CORRUPT, TRUNCATED, SKIP = 0, 1, 2, 4, 8       # CRNN_JPEG_* (include/crnn_mi355x.h)
QUANT_INTS, HUFF_INTS, POOL_INTS_PER_FILE = 64, 548, 3480

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
                   56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

_L, _I = np.dtype("l"), np.intc
ITEM_DTYPE = np.dtype([("data_off", _L), ("scan_off", _L), ("scan_end", _L), ("page_off", _L), ("samp_off", _L), ("rows", _I), ("cols", _I),
                       ("stride", _I), ("ncomp", _I), ("hs", _I, 3), ("vs", _I, 3), ("qt", _I, 3), ("dc", _I, 3), ("ac", _I, 3), ("restart", _I),
                       ("mcux", _I), ("mcuy", _I), ("seg0", _I), ("nseg", _I), ("status", _I)], align=True)
SEG_DTYPE = np.dtype([("begin", _L), ("end", _L), ("item", _I), ("mcu0", _I), ("nmcu", _I), ("pad", _I)], align=True)


class crnn_jpeg_item(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_jpeg_item."""
    _fields_ = ([(n, ctypes.c_long) for n in ("data_off", "scan_off", "scan_end", "page_off", "samp_off")]
                + [(n, ctypes.c_int) for n in ("rows", "cols", "stride", "ncomp")]
                + [(n, ctypes.c_int * 3) for n in ("hs", "vs", "qt", "dc", "ac")]
                + [(n, ctypes.c_int) for n in ("restart", "mcux", "mcuy", "seg0", "nseg", "status")])


class crnn_jpeg_seg(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_jpeg_seg."""
    _fields_ = [("begin", ctypes.c_long), ("end", ctypes.c_long)] + [(n, ctypes.c_int) for n in ("item", "mcu0", "nmcu", "pad")]


assert ITEM_DTYPE.itemsize == ctypes.sizeof(crnn_jpeg_item) and SEG_DTYPE.itemsize == ctypes.sizeof(crnn_jpeg_seg)


# ---------------------------------------------------------------- the headers ----------------------------------------------------------------

def header_size(data):
    """(rows, cols) from the first frame header of a JPEG file's bytes, or None when there is none to be found (not a JPEG, or cut short)."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    p, n = 2, len(data)
    while p + 4 <= n:
        if data[p] != 0xFF:
            return None
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            p += 2
            continue
        L = (data[p + 2] << 8) | data[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if p + 9 > n:
                return None
            return ((data[p + 5] << 8) | data[p + 6]), ((data[p + 7] << 8) | data[p + 8])
        if m in (0xDA, 0xD9) or L < 2:
            return None
        p += 2 + L
    return None


def _huff_table(counts, symbols):
    """The canonical table of the pool: maxcode[18], valoff[18], 256 symbols, the 8-bit look-ahead; None when the counts overflow the code space."""
    t = [0] * HUFF_INTS
    t[0] = t[17] = -1
    code = k = 0
    for l in range(1, 17):
        t[18 + l] = k - code
        code += counts[l - 1]
        if code > (1 << l):
            return None
        t[l] = code - 1 if counts[l - 1] else -1
        k += counts[l - 1]
        code <<= 1
    t[36:36 + len(symbols)] = symbols
    for pre in range(256):                      # the look-ahead: what the length search finds within 8 bits
        for l in range(1, 9):
            if (pre >> (8 - l)) <= t[l]:
                t[292 + pre] = (l << 8) | t[36 + ((t[18 + l] + (pre >> (8 - l))) & 255)]
                break
    return np.array(t, np.int32)


def parse_jpeg(data):
    """The Python twin of crnn_jpeg_plan for one file's bytes -> dict: status, and as far as they were reached rows, cols, ncomp; for a supported
    file also hs, vs, quant (per component, 64 int32 in natural order), dc / ac (per component, the pool's Huffman table), restart, mcux, mcuy,
    scan_off, scan_end and segs = [(begin, end, mcu0, nmcu)] (offsets into data)."""
    d, n = bytes(data), len(data)
    out = dict(status=UNSUPPORTED, rows=0, cols=0, ncomp=0)

    def done(status):
        out["status"] = status
        return out

    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        return done(UNSUPPORTED)
    q, q16, huff = {}, {}, {}
    frame, jfif, adobe, restart, p = None, False, None, 0, 2
    while True:
        if p >= n or d[p] != 0xFF:
            return done(CORRUPT)
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            return done(CORRUPT)
        m = d[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD9, 0xD8, 0x00) or p + 2 > n:
            return done(CORRUPT)
        L = (d[p] << 8) | d[p + 1]
        if L < 2 or p + L > n:
            return done(CORRUPT)
        s = d[p + 2:p + L]
        k = len(s)
        if m == 0xDB:
            o = 0
            while o < k:
                pq, tq = s[o] >> 4, s[o] & 15
                if pq > 1 or tq > 3 or o + 1 + 64 * (pq + 1) > k:
                    return done(CORRUPT)
                vals = np.frombuffer(s, dtype=">u2" if pq else np.uint8, count=64, offset=o + 1).astype(np.int32)
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = vals
                q[tq], q16[tq] = t, bool(pq)
                o += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            o = 0
            while o < k:
                if o + 17 > k or (s[o] >> 4) > 1 or (s[o] & 15) > 3:
                    return done(CORRUPT)
                counts = list(s[o + 1:o + 17])
                total = sum(counts)
                if _huff_table(counts, []) is None or total > 256 or o + 17 + total > k:
                    return done(CORRUPT)
                t = _huff_table(counts, list(s[o + 17:o + 17 + total]))
                huff[(s[o] >> 4, s[o] & 15)] = t
                o += 17 + total
        elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):
            if frame is not None or k < 6:
                return done(CORRUPT)
            prec, rows, cols, nc = s[0], (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if k != 6 + 3 * nc or rows == 0 or cols == 0 or nc == 0:
                return done(CORRUPT)
            out.update(rows=rows, cols=cols, ncomp=nc)
            if m > 0xC1 or prec != 8 or nc not in (1, 3):
                return done(UNSUPPORTED)
            frame = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(nc)]
            if any(not (1 <= h <= 4 and 1 <= v <= 4 and t <= 3) for _, h, v, t in frame):
                return done(CORRUPT)
        elif m == 0xDD:
            if k != 2:
                return done(CORRUPT)
            restart = (s[0] << 8) | s[1]
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            if k >= 12 and s[:5] == b"Adobe":
                adobe = s[11]
        elif m == 0xDA:
            if frame is None or k < 1:
                return done(CORRUPT)
            ns = s[0]
            if ns < 1 or ns > 4 or k != 4 + 2 * ns:
                return done(CORRUPT)
            if ns != len(frame):
                return done(UNSUPPORTED)
            td, ta = [], []
            for c in range(ns):
                if s[1 + 2 * c] != frame[c][0]:
                    return done(UNSUPPORTED)
                td.append(s[2 + 2 * c] >> 4)
                ta.append(s[2 + 2 * c] & 15)
                if td[-1] > 3 or ta[-1] > 3:
                    return done(CORRUPT)
            if s[1 + 2 * ns] != 0 or s[2 + 2 * ns] != 63 or s[3 + 2 * ns] != 0:
                return done(UNSUPPORTED)
            hs, vs = [f[1] for f in frame], [f[2] for f in frame]
            if ns == 1:
                hs, vs = [1], [1]
            else:
                if (hs[0], vs[0]) not in ((1, 1), (2, 1), (2, 2)) or (hs[1], vs[1], hs[2], vs[2]) != (1, 1, 1, 1):
                    return done(UNSUPPORTED)
                ids = bytes(f[0] for f in frame)
                if (adobe == 0) if adobe is not None else (not jfif and ids == b"RGB"):
                    return done(UNSUPPORTED)
            for c in range(ns):
                if frame[c][3] not in q or (0, td[c]) not in huff or (1, ta[c]) not in huff:
                    return done(CORRUPT)
                if q16[frame[c][3]]:
                    return done(UNSUPPORTED)
            rows, cols = out["rows"], out["cols"]
            mcux, mcuy = -(-cols // (8 * hs[0])), -(-rows // (8 * vs[0]))
            nmcu = mcux * mcuy
            expect = -(-nmcu // restart) if restart else 1
            scan_off = p + L
            pos, seg_begin, scan_end, end_marker, bounds = scan_off, scan_off, n, None, []
            while pos < n:
                ff = d.find(b"\xff", pos)
                if ff < 0:
                    break
                pos = ff
                while pos + 1 < n and d[pos + 1] == 0xFF:
                    pos += 1
                if pos + 1 >= n:
                    scan_end = ff
                    break
                c = d[pos + 1]
                pos += 2
                if c == 0:
                    continue
                if restart and 0xD0 <= c <= 0xD7:
                    bounds.append((seg_begin, ff))
                    seg_begin = pos
                    continue
                scan_end, end_marker = ff, c
                break
            if end_marker is not None and end_marker != 0xD9:
                return done(UNSUPPORTED)
            bounds.append((min(seg_begin, scan_end), scan_end))
            bounds = bounds[:expect] + [(scan_end, scan_end)] * (expect - len(bounds))
            step = restart if restart else nmcu
            out.update(ncomp=ns, hs=hs, vs=vs, restart=restart, mcux=mcux, mcuy=mcuy, scan_off=scan_off, scan_end=scan_end,
                       quant=[q[f[3]] for f in frame], dc=[huff[(0, t)] for t in td], ac=[huff[(1, t)] for t in ta],
                       segs=[(b, e, i * step, min(step, nmcu - i * step)) for i, (b, e) in enumerate(bounds)])
            return done(OK)
        p += L


# ---------------------------------------------------------------- the host definition ----------------------------------------------------------------

class _Bits:
    """A segment's bits after byte unstuffing (FF xx -> FF), followed by zeros without end; `pos` counts the bits consumed."""

    def __init__(self, seg):
        out, i, n = bytearray(), 0, len(seg)
        while i < n:
            b = seg[i]
            i += 1
            out.append(b)
            if b == 0xFF:
                i += 1
        self.nbits, self.pos = 8 * len(out), 0
        self.buf = bytes(out) + b"\0\0\0"

    def peek16(self):
        k = self.pos >> 3
        if k + 3 > len(self.buf):
            return 0
        w = (self.buf[k] << 16) | (self.buf[k + 1] << 8) | self.buf[k + 2]
        return (w >> (8 - (self.pos & 7))) & 0xFFFF

    def symbol(self, tab):
        v = self.peek16()
        for l in range(1, 17):
            if (v >> (16 - l)) <= tab[l]:
                self.pos += l
                return int(tab[36 + ((int(tab[18 + l]) + (v >> (16 - l))) & 255)]) & 255
        return -1

    def receive_extend(self, s):
        v = self.peek16() >> (16 - s)
        self.pos += s
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _wrap16(v):
    return ((v + 0x8000) & 0xFFFF) - 0x8000


def _entropy(d, info):
    """-> (per component the coefficients [blocks down][blocks across][64] int64 in natural order, status bits), segment by segment."""
    hs, vs, mcux, mcuy = info["hs"], info["vs"], info["mcux"], info["mcuy"]
    nc = info["ncomp"]
    coef = [np.zeros((mcuy * vs[c], mcux * hs[c], 64), np.int64) for c in range(nc)]
    dc = [[int(x) for x in t] for t in info["dc"]]
    ac = [[int(x) for x in t] for t in info["ac"]]
    zz = [int(z) for z in ZIGZAG]
    status = 0
    for begin, end, mcu0, nmcu in info["segs"]:
        br = _Bits(d[begin:end])
        pred = [0] * nc
        bad = False
        for mcu in range(mcu0, mcu0 + nmcu):
            my, mx = divmod(mcu, mcux)
            for c in range(nc):
                for bv in range(vs[c]):
                    for bh in range(hs[c]):
                        o = coef[c][my * vs[c] + bv, mx * hs[c] + bh]
                        s = br.symbol(dc[c])
                        if s < 0 or s > 11:
                            bad = True
                            break
                        if s:
                            pred[c] += br.receive_extend(s)
                        o[0] = _wrap16(pred[c])
                        k = 1
                        while k < 64:
                            rs = br.symbol(ac[c])
                            if rs < 0:
                                bad = True
                                break
                            r, sz = rs >> 4, rs & 15
                            if sz == 0 and r != 15:
                                break
                            if k + r > 63:
                                bad = True
                                break
                            k += r
                            if sz:
                                o[zz[k]] = br.receive_extend(sz)
                            k += 1
                        if bad:
                            break
                    if bad:
                        break
                if bad:
                    break
            if bad:
                break
        status |= (CORRUPT if bad else 0) | (TRUNCATED if br.pos > br.nbits else 0)
    return coef, status


def _wrap32(x):
    return x.astype(np.int32).astype(np.int64)


def _idct_pass(i):
    """jidctint's 1-D pass over the first axis of i (8, ...) int64."""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) * 8192, (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3])


def _idct_plane(coef, quant):
    """[by][bx][64] coefficients -> the (8 by, 8 bx) uint8 plane: dequantise, columns, rows, + 128, clamp; int32 wrap-around where the kernel wraps."""
    nby, nbx = coef.shape[:2]
    x = _wrap32(coef * quant.astype(np.int64)).reshape(nby, nbx, 8, 8)                # [by][bx][row][col]
    x = _wrap32(_idct_pass(np.moveaxis(x, 2, 0)))                                      # columns: along the row index
    x = _wrap32(x + 1024) >> 11
    x = np.moveaxis(x, 0, 2)
    x = _wrap32(_idct_pass(np.moveaxis(x, 3, 0)))                                      # rows: along the column index
    x = (_wrap32(x + (1 << 17)) >> 18) + 128
    x = np.clip(np.moveaxis(x, 0, 3), 0, 255)
    return x.transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8).astype(np.uint8)


def _upsample(plane, hs, vs, dw, dh, rows, cols):
    """libjpeg's "fancy" upsampling of a chroma plane (the component's dh x dw samples) by hs x vs, cropped to rows x cols; int64."""
    p = plane[:dh, :dw].astype(np.int64)
    if hs == 1:
        return p[:rows, :cols]
    if vs == 2:
        if dw <= 2:
            return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:rows, :cols]
        r = np.arange(2 * dh)
        near = r >> 1
        far = np.clip(np.where(r & 1, near + 1, near - 1), 0, dh - 1)
        s, bias_e, bias_o, edge, sh = 3 * p[near] + p[far], 8, 7, 4, 4
    else:
        if dw <= 2:
            return np.repeat(p, 2, axis=1)[:rows, :cols]
        s, bias_e, bias_o, edge, sh = p, 1, 2, 1, 2
    out = np.empty((s.shape[0], 2 * dw), np.int64)
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out[:, 0::2] = (3 * s + left + bias_e) >> sh
    out[:, 1::2] = (3 * s + right + bias_o) >> sh
    if vs == 2:
        out[:, 0], out[:, -1] = (edge * s[:, 0] + bias_e) >> sh, (edge * s[:, -1] + bias_o) >> sh
    else:
        out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out[:rows, :cols]


def jpeg_decode_host(data):
    """The definition the kernels are held to.  data: a JPEG file's bytes -> (planes, status): (H, W, 3) uint8 RGB, or (H, W) uint8 for a
    one-component file; status as the library reports it (0, or a sum of UNSUPPORTED / CORRUPT / TRUNCATED).  A non-zero status gives zero planes
    of the header's size (None when no frame header was reached): the device zero-fills such a page too.  A truncated file is decoded with zero
    bits after its end, which sets TRUNCATED; a scan that a restart interval cuts into segments loses only the segments that run out."""
    d = bytes(data)
    info = parse_jpeg(d)
    status, rows, cols = info["status"], info["rows"], info["cols"]
    grey = info["ncomp"] == 1
    if status == OK:
        coef, status = _entropy(d, info)
    if status != OK:
        return (np.zeros((rows, cols) if grey else (rows, cols, 3), np.uint8) if rows and cols else None), status
    planes = [_idct_plane(coef[c], info["quant"][c]) for c in range(info["ncomp"])]
    if grey:
        return np.ascontiguousarray(planes[0][:rows, :cols]), OK
    hs, vs = info["hs"][0], info["vs"][0]
    dw, dh = -(-cols // hs), -(-rows // vs)
    y = planes[0][:rows, :cols].astype(np.int64)
    cb = _upsample(planes[1], hs, vs, dw, dh, rows, cols) - 128
    cr = _upsample(planes[2], hs, vs, dw, dh, rows, cols) - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8), OK


_TIES = None


def _fma(a, b, c):
    """The correctly rounded float64 of a * b + c (Fraction arithmetic is exact; int / int division rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def tie_table():
    """-> (keys, grey): the 16 782 triples R << 16 | G << 8 | B (sorted) at which 299 R + 587 G + 114 B + 500 is a multiple of 1000, and the
    grey the FMA rule gives there.  Built once."""
    global _TIES
    if _TIES is None:
        r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
        at = np.flatnonzero((299 * r + 587 * g + 114 * b + 500).ravel() % 1000 == 0)
        grey = np.empty(len(at), np.uint8)
        for k, key in enumerate(at):
            R, G, B = int(key) >> 16, (int(key) >> 8) & 255, int(key) & 255
            grey[k] = int(np.floor(_fma(0.114, float(B), _fma(0.587, float(G), 0.299 * float(R))) + 0.5))
        _TIES = (at.astype(np.int64), grey)
    return _TIES


def gray_of_rgb(rgb):
    """(..., 3) uint8 -> (...) uint8 by the FMA rule: (299 R + 587 G + 114 B + 500) // 1000 off the ties, the tie table on them."""
    v = rgb.astype(np.int64)
    total = 299 * v[..., 0] + 587 * v[..., 1] + 114 * v[..., 2] + 500
    grey = (total // 1000).astype(np.uint8)
    tie = total % 1000 == 0
    if tie.any():
        keys, table = tie_table()
        key = (v[..., 0] << 16 | v[..., 1] << 8 | v[..., 2])[tie]
        grey[tie] = table[np.searchsorted(keys, key)]
    return grey


def jpeg_gray_host(data):
    """A JPEG file's bytes -> the (H, W) uint8 grey page the device writes (zeros when the status is not 0); ValueError without a frame header."""
    planes, status = jpeg_decode_host(data)
    if planes is None:
        raise ValueError("no JPEG frame header (status %d)" % status)
    return planes if planes.ndim == 2 else gray_of_rgb(planes)


# ---------------------------------------------------------------- the plan and the device ----------------------------------------------------------------

def plan(datas):
    """crnn_jpeg_plan over a list of byte strings -> (blob uint8, items ITEM_DTYPE, segs SEG_DTYPE, pool int32, totals): no GPU call."""
    L = native.lib()
    n = len(datas)
    lens = np.array([len(x) for x in datas], dtype=_L)
    offs = np.zeros(n, dtype=_L)
    if n:
        offs[1:] = np.cumsum(lens)[:-1]
    blob = np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)
    items = np.zeros(n, ITEM_DTYPE)
    pool = np.empty(max(n, 1) * POOL_INTS_PER_FILE, np.int32)
    totals = np.zeros(4, dtype=_L)
    cap = n + int(lens.sum()) // 256

    def call(segs):
        return L.crnn_jpeg_plan(blob.ctypes.data, int(lens.sum()), offs.ctypes.data, lens.ctypes.data, n, items.ctypes.data, pool.ctypes.data, len(pool),
                                segs.ctypes.data, len(segs), totals.ctypes.data)
    segs = np.zeros(max(cap, 1), SEG_DTYPE)
    code = call(segs)
    if code == -2 and totals[1] > len(segs):          # the segment table was a guess: once more at the size the plan asks for
        segs = np.zeros(int(totals[1]), SEG_DTYPE)
        code = call(segs)
    native.check(code, "jpeg_plan")
    return blob, items, segs[:int(totals[1])], pool[:int(totals[0])], totals


def _up16(n):
    return -(-int(n) // _ARENA_ALIGN) * _ARENA_ALIGN


class JpegDecoder:
    """Image files -> grey pages on the device.  decode() reads the headers on the host (crnn_jpeg_plan), uploads the files' bytes with the plan's
    tables in ONE page-locked copy and runs crnn_jpeg_decode's three launches on the current stream; nothing is read back.  Files the plan marks
    unsupported (progressive, CMYK, ... and everything that is no JPEG: PNG) and files with more than `max_segment_bytes` of entropy-coded data
    per segment (one lane decodes a segment serially) are decoded by data.read_img on the host; their grey bytes travel in the same upload into
    their arena slots, so a mixed folder works.  The default of max_segment_bytes is a PLACEHOLDER (64 KiB: every one-word file, no page without
    restart markers); scripts/jpeg_bench.py measures both sides of it.  Two staging slots, as DeviceIngest: successive calls belong on one
    stream."""

    def __init__(self, device=None, max_segment_bytes=64 << 10):
        self.lib, self.device = device_lib("JpegDecoder", "jpeg.jpeg_gray_host", device)
        self.max_segment_bytes = int(max_segment_bytes)
        self._slot = StagingSlots(self.device, 2).take

    def decode(self, files):
        """files: byte strings or file names -> (PageArena, status, shapes).  status: device int32 per file -- 0 decoded on the device (or on the
        host because of its size), UNSUPPORTED (1) decoded on the host, CORRUPT (2) / TRUNCATED (4) a zero page (a file without a readable frame
        header: a 1 x 1 zero page).  shapes: [(rows, cols)].  The arena's host side is None and its `pages` are shape-only placeholders."""
        import torch
        from .data import read_img
        from .engine import _stream
        datas = []
        for f in files:
            if isinstance(f, (bytes, bytearray, memoryview)):
                datas.append(bytes(f))
            else:
                with open(f, "rb") as fh:
                    datas.append(fh.read())
        n = len(datas)
        if n == 0:
            raise ValueError("no files to decode")
        blob, items, segs, pool, _ = plan(datas)
        host_pages = {}
        per_seg = (items["scan_end"] - items["scan_off"]) // np.maximum(items["nseg"], 1)
        for i in range(n):
            st = int(items["status"][i])
            if st == UNSUPPORTED or (st == OK and per_seg[i] > self.max_segment_bytes):
                host_pages[i] = np.ascontiguousarray(read_img(io.BytesIO(datas[i])))
                items["rows"][i], items["cols"][i] = host_pages[i].shape
                if st == OK:
                    items["status"][i] = SKIP
            elif st != OK and (items["rows"][i] < 1 or items["cols"][i] < 1):
                items["rows"][i] = items["cols"][i] = 1
        # the layout: every file a page, back to back on 16-byte boundaries (pages.arena_layout); samples for the device's files only
        sizes = items["rows"].astype(np.int64) * items["cols"]
        padded = (sizes + _ARENA_ALIGN - 1) // _ARENA_ALIGN * _ARENA_ALIGN
        offs = np.concatenate([[0], np.cumsum(padded)[:-1]])
        nbytes = int(padded.sum())
        items["page_off"], items["stride"] = offs, items["cols"]
        live = items["status"] == OK
        samp = np.where(live, sum(items["mcux"].astype(np.int64) * items["hs"][:, c] * 8 * items["mcuy"] * items["vs"][:, c] * 8 for c in range(3)), 0)
        items["samp_off"] = np.concatenate([[0], np.cumsum(samp)[:-1]])
        samples = int(samp.sum())
        shapes = [(int(r), int(c)) for r, c in zip(items["rows"], items["cols"])]
        # one upload: [the arena's image, when the host decoded some of it] blob | items | segs | pool
        parts = [blob, items.view(np.uint8), segs.view(np.uint8), pool.view(np.uint8)]
        a0 = _up16(nbytes) if host_pages else 0
        starts, pos = [], a0
        for part in parts:
            starts.append(pos)
            pos = _up16(pos + part.nbytes)
        with torch.cuda.device(self.device):
            s = self._slot(max(pos, 1))
            if host_pages:
                s["np"][:a0] = 0
                for i, pg in host_pages.items():
                    s["np"][offs[i]:offs[i] + pg.size] = pg.ravel()
            for part, at in zip(parts, starts):
                s["np"][at:at + part.nbytes] = part.reshape(-1)
            s["dev"][:pos].copy_(s["host"][:pos], non_blocking=True)
            s["copied"].record(torch.cuda.current_stream())
            arena = s["dev"][:max(nbytes, 1)].clone() if host_pages else torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=self.device)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            ws_bytes = int(self.lib.crnn_jpeg_workspace_bytes(samples))
            ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=self.device)
            base = s["dev"].data_ptr()
            native.check(self.lib.crnn_jpeg_decode(base + starts[0], blob.nbytes, items.ctypes.data, base + starts[1], n, segs.ctypes.data,
                                                   base + starts[2], len(segs), base + starts[3], len(pool), arena.data_ptr(), nbytes, status.data_ptr(),
                                                   ws.data_ptr(), ws_bytes, _stream()), "jpeg_decode")
        pages = [np.broadcast_to(np.uint8(0), sh) for sh in shapes]           # shape-only: the pixels live on the device
        return PageArena(pages, [int(o) for o in offs], nbytes, None, arena), status, shapes
