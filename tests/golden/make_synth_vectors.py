#!/usr/bin/env python3
"""The pinned vectors of tests/test_synth_cpu.py: the rule of crnn_synth_words as include/crnn_mi355x.h words it, in plain Python loops over
Python integers -- written from the header's text, not from crnn_mi355x.synth (it imports nothing of the package).  Prints the expected
bytes of every case; they are pasted into the test.  usage: make_synth_vectors.py"""

T0, T1 = 6, 4
# two faces of three glyphs: (bitmap rows, left, top, advance); face 0 holds 3 x 2 glyphs (w = 3, h = 2), face 1 holds 2 x 3 glyphs
FACES = [
    [([[10, 20, 30], [40, 50, 60]], 0, 1, 3), ([[70, 80, 90], [100, 110, 120]], 1, 0, 4), ([[130, 140, 150], [160, 170, 255]], -1, 2, 2)],
    [([[15, 25], [35, 45], [55, 65]], 0, 0, 2), ([[75, 85], [95, 105], [115, 125]], 0, 1, 3), (None, 0, 0, 2)],
]
# (name, codes, item)
CASES = [
    ("identity", [0, 1], dict(face=0, track=0, jitter=0, sx=65536, sy=65536, ox=0, oy=0, fg=255, bg=0, seed=0)),
    ("fractional offset", [0, 1], dict(face=0, track=0, jitter=0, sx=65536, sy=65536, ox=-40000, oy=25000, fg=255, bg=0, seed=0)),
    ("negative track, overlap", [1, 0, 2], dict(face=0, track=-3, jitter=0, sx=65536, sy=65536, ox=0, oy=0, fg=255, bg=0, seed=0)),
    ("jitter", [0, 1, 0], dict(face=1, track=0, jitter=2, sx=65536, sy=65536, ox=0, oy=-65536, fg=255, bg=0, seed=77)),
    ("dark ink on a bright ground", [1, 2], dict(face=0, track=1, jitter=0, sx=50000, sy=80000, ox=30000, oy=-20000, fg=20, bg=230, seed=0)),
    ("empty word", [], dict(face=1, track=2, jitter=1, sx=65536, sy=65536, ox=0, oy=0, fg=200, bg=33, seed=5)),
    ("scaled, jittered, a glyph without ink", [0, 2, 1], dict(face=1, track=1, jitter=1, sx=90000, sy=70000, ox=-70000, oy=10000, fg=250, bg=5,
                                                              seed=123456789)),
]
M32 = 0xffffffff


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def render(codes, it):
    face = FACES[it["face"]]
    placed, pen = [], 0
    for k, code in enumerate(codes):
        bitmap, left, top, advance = face[code]
        h = mix32(it["seed"] ^ ((k * 0x9E3779B9) & M32))
        dy = (((h & 0xffff) * (2 * it["jitter"] + 1)) >> 16) - it["jitter"]
        placed.append((bitmap, pen + left, top + dy))
        pen += advance + it["track"]

    def cov(x, y):
        best = 0
        for bitmap, gx, gy in placed:
            if bitmap is None:
                continue
            r, c = y - gy, x - gx
            if 0 <= r < len(bitmap) and 0 <= c < len(bitmap[0]):
                best = max(best, bitmap[r][c])
        return best

    out = [[0] * T1 for _ in range(T0)]
    for i in range(T0):
        for j in range(T1):
            X = it["sx"] * i + it["ox"]                       # Python integers: >> floors
            Y = it["sy"] * (T1 - 1 - j) + it["oy"]
            x0, fx, y0, fy = X >> 16, (X >> 8) & 255, Y >> 16, (Y >> 8) & 255
            c = ((256 - fy) * (256 - fx) * cov(x0, y0) + (256 - fy) * fx * cov(x0 + 1, y0) + fy * (256 - fx) * cov(x0, y0 + 1)
                 + fy * fx * cov(x0 + 1, y0 + 1) + 32768) >> 16
            out[i][j] = (it["bg"] * (255 - c) + it["fg"] * c + 127) // 255
    return out


if __name__ == "__main__":
    for name, codes, it in CASES:
        print("    %r,      # %s" % (render(codes, it), name))
