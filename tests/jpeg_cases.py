"""The JPEG fixtures of tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py, encoded by Pillow from seeded arrays: 9 sizes x 2 images x 4
samplings x 4 encoder settings = 288 files, built once per process."""
import io

import numpy as np

SIZES = [(31, 97), (32, 100), (1, 1), (7, 3), (17, 5), (9, 33), (16, 16), (33, 18), (2, 70)]            # (H, W)
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
SETTINGS = [dict(quality=75), dict(quality=95, optimize=True), dict(quality=30, restart_marker_blocks=1), dict(quality=100)]
_GRID = None


def _images(h, w, seed):
    rs = np.random.RandomState(seed)
    noise = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    walk = rs.randint(-6, 7, (h, w, 3)).cumsum(axis=0).cumsum(axis=1) // 4 + rs.randint(60, 200, 3)
    return [("noise", noise), ("walk", np.clip(walk, 0, 255).astype(np.uint8))]


def encode(arr, sampling="4:2:0", **settings):
    from PIL import Image
    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(np.ascontiguousarray(arr[..., 1] if arr.ndim == 3 else arr), "L").save(buf, "JPEG", **settings)
    else:
        Image.fromarray(arr, "RGB").save(buf, "JPEG", subsampling=sampling, **settings)
    return buf.getvalue()


def grid():
    """-> [(id, bytes)]: the 288 files."""
    global _GRID
    if _GRID is None:
        _GRID = []
        for k, (h, w) in enumerate(SIZES):
            for kind, arr in _images(h, w, 100 + k):
                for sampling in SAMPLINGS:
                    for j, st in enumerate(SETTINGS):
                        _GRID.append(("%dx%d-%s-%s-s%d" % (h, w, kind, sampling, j), encode(arr, sampling, **st)))
    return _GRID


def pillow(data, mode):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert(mode))
