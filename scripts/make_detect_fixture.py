#!/usr/bin/env python3
"""Draws tests/golden/detect_page.npz, the rendered page of the word-detection tests: three lines of words (4 + 3 + 4) in Pillow's built-in
font (FreeType, size 10), dark on light, with exactly GAP = 13 background columns between the ink of neighbouring words.  Stored: `page`
(uint8), `boxes` (11, 4) int32 = r0 r1 c0 c1 of each word's ink in reading order, `words`.  The truth is independent of the detector: every
word is rendered alone and thresholded at <= 127; its tight ink box, moved to where the word is pasted, is its truth.  The words avoid
letters with detached parts (i, j): with gap_y = 0 a dot is a component of its own.  The tests read the file and never render.

    python scripts/make_detect_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

LINES = [["word", "boxes", "from", "pages"], ["forward", "beam", "search"], ["one", "upload", "small", "reads"]]
GAP, MARGIN, LINE_STEP, SIZE = 13, 9, 17, 10


def render(word):
    """-> (the word alone on a light canvas (uint8), its tight ink box r0 r1 c0 c1 at threshold <= 127)."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size=SIZE)
    img = Image.new("L", (12 * len(word) + 8, 2 * SIZE + 4), 255)
    ImageDraw.Draw(img).text((4, 2), word, fill=0, font=font)
    a = np.array(img, dtype=np.uint8)
    rr, cc = np.nonzero(a <= 127)
    return a, (int(rr.min()), int(rr.max()) + 1, int(cc.min()), int(cc.max()) + 1)


def main(out):
    drawn = [[render(w) for w in line] for line in LINES]
    width = MARGIN + max(sum(b[3] - b[2] for _, b in line) + GAP * (len(line) - 1) for line in drawn) + MARGIN
    height = MARGIN + LINE_STEP * len(LINES) + MARGIN
    page = np.full((height, width), 255, np.uint8)
    boxes = []
    for k, line in enumerate(drawn):
        y, x = MARGIN + LINE_STEP * k, MARGIN
        for a, (r0, r1, c0, c1) in line:
            w = c1 - c0
            page[y:y + a.shape[0], x:x + w] = np.minimum(page[y:y + a.shape[0], x:x + w], a[:, c0:c1])   # the ink's columns only
            boxes.append((y + r0, y + r1, x, x + w))
            x += w + GAP
    np.savez_compressed(out, page=page, boxes=np.array(boxes, np.int32), words=np.array([w for line in LINES for w in line]))
    print("wrote %s: page %d x %d, %d words, %d bytes" % (out, height, width, len(boxes), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "detect_page.npz"))
