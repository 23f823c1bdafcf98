"""Writes tests/golden/jpeg/: a handful of small JPEG files and, in expected.npz, the RGB (or Y) planes libjpeg-turbo decodes from them -- so that
tests/test_jpeg_cpu.py pins crnn_mi355x.jpeg.jpeg_decode_host where the local Pillow has another JPEG library or none.  Run from the repository
root with a Pillow that has libjpeg-turbo; the planes come from Pillow alone, not from the code under test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases as JC  # noqa: E402

PICKS = [((31, 97), "walk", "4:2:0", dict(quality=75)), ((17, 5), "noise", "4:2:2", dict(quality=95, optimize=True)),
         ((9, 33), "walk", "4:4:4", dict(quality=100)), ((33, 18), "walk", "grey", dict(quality=30, restart_marker_blocks=1)),
         ((2, 70), "noise", "4:2:0", dict(quality=30, restart_marker_blocks=1)), ((7, 3), "walk", "4:2:0", dict(quality=75))]

if __name__ == "__main__":
    from PIL import features
    assert features.check("libjpeg_turbo"), "the expected planes are libjpeg-turbo's"
    out = os.path.join(HERE, "jpeg")
    os.makedirs(out, exist_ok=True)
    expected = {}
    for k, ((h, w), kind, sampling, st) in enumerate(PICKS):
        arr = dict(JC._images(h, w, 100 + JC.SIZES.index((h, w))))[kind]
        data = JC.encode(arr, sampling, **st)
        name = "g%d_%dx%d_%s.jpg" % (k, h, w, sampling.replace(":", ""))
        open(os.path.join(out, name), "wb").write(data)
        planes = JC.pillow(data, "L" if sampling == "grey" else "RGB")
        expected[name] = planes
        # the grey page: read_img's expression on an (N, 1, 3) array, the summation path the FMA rule of crnn_mi355x/jpeg.py restates
        expected[name + ":grey"] = planes if planes.ndim == 2 else np.clip(np.floor(
            planes.reshape(-1, 1, 3).astype(np.float64) @ np.array([0.299, 0.587, 0.114]) + 0.5), 0, 255).astype(np.uint8).reshape(planes.shape[:2])
    np.savez_compressed(os.path.join(out, "expected.npz"), **expected)
    print("wrote", sorted(expected))
