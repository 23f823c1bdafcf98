"""Page deskew on the host (crnn_mi355x/deskew.py): the two rules against the brute-force restatement of tests/deskew_ref.py (one pixel at a
time in Python integers), the tie rule, the validation, the skewed page on which the reading order of the raw boxes is wrong -- the reason for
the feature -- and the source list and flags.  Everything is integer: every comparison is exact equality."""
import os
import sys

import numpy as np
import pytest

from crnn_mi355x import deskew as K, detect as D, native
import deskew_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
SHAPES = [(1, 1), (1, 23), (19, 1), (8, 12), (13, 17)]       # 1 x 1, 1 x N, N x 1, even and odd sizes


@pytest.mark.parametrize("shape", SHAPES)
def test_scores_equal_the_brute_force_rule(shape):
    for polarity, dark in ((1, True), (2, False), (0, True)):
        page = R.sparse_ink(*shape, seed=shape[0] + shape[1] + polarity, dark=dark)
        ink = R.ink_brute(page, 127, polarity)
        assert np.array_equal(np.array(ink), D.ink_mask(page, 127, polarity)[0])
        for steps in (0, 1, 64):
            index, scores = K.estimate_skew_host(page, threshold=127, polarity=polarity, steps=steps, slope_step=256)
            want = R.scores_brute(ink, steps, 256)
            assert scores.dtype == np.int64 and scores.tolist() == want, (shape, polarity, steps)
            assert index == R.pick_brute(want)
            assert np.array_equal(K.skew_scores_host(page, 127, polarity, steps, 256), scores)
    page = R.sparse_ink(*shape, seed=5)
    assert K.skew_scores_host(page, 127, 1, 16, 1024).tolist() == R.scores_brute(R.ink_brute(page, 127, 1), 16, 1024)   # the steepest slope


def test_otsu_ink_is_the_detectors():
    page = R.sparse_ink(20, 31, seed=2)
    ink, t, dark = D.ink_mask(page)
    assert 60 <= t < 200 and dark == 1
    assert K.skew_scores_host(page, steps=8).tolist() == R.scores_brute(ink.tolist(), 8, 256)
    assert K.skew_scores_host(255 - page, steps=8).tolist() == K.skew_scores_host(page, steps=8).tolist()    # the auto polarity


@pytest.mark.parametrize("shape", SHAPES)
def test_rotation_equals_the_brute_force_rule(shape):
    page = R.random_grey(*shape, seed=shape[0] * 3 + shape[1])
    for fill in (-1, 0, 255, 77):
        for index in (-64, -37, -1, 0, 1, 20, 64):
            got = K.rotate_host(page, index, 256, fill)
            assert got.dtype == np.uint8 and got.shape == page.shape
            assert np.array_equal(got, R.rotate_brute(page, index, 256, fill)), (shape, fill, index)
    assert np.array_equal(K.rotate_host(page, 16, 1024, -1), R.rotate_brute(page, 16, 1024, -1))
    assert np.array_equal(K.rotate_host(page, -5, 3, 9), R.rotate_brute(page, -5, 3, 9))


def test_index_zero_is_the_identity():
    for shape in SHAPES + [(40, 50)]:
        page = R.random_grey(*shape, seed=7)
        for fill in (-1, 0, 255):
            assert np.array_equal(K.rotate_host(page, 0, 256, fill), page)
    assert K.rotation_pair(0) == (65536, 0) and K.rotation_pair(64, 256) == (63579, 15895) and K.rotation_pair(-64, 256) == (63579, -15895)
    assert K.slope_of(48) == 0.1875 and abs(K.angle_of(48) - 10.6197) < 1e-3 and K.angle_of(-48) == -K.angle_of(48)


def test_the_tie_rule():
    one = np.full((9, 12), 255, np.uint8)
    one[4, 2] = 0
    index, scores = K.estimate_skew_host(one, threshold=127, polarity=1, steps=64)
    assert index == 0 and scores.tolist() == [1] * 129                       # every candidate scores 1: the smallest |a|
    for page in (np.full((9, 12), 255, np.uint8), np.full((9, 12), 131, np.uint8)):
        for kw in (dict(threshold=127, polarity=1), dict()):                 # blank under a threshold, constant under Otsu: no ink
            index, scores = K.estimate_skew_host(page, steps=5, **kw)
            assert index == 0 and scores.tolist() == [0] * 11
    full = np.zeros((9, 12), np.uint8)
    index, scores = K.estimate_skew_host(full, threshold=127, polarity=1, steps=64)
    assert index == 0 and scores[64] == 9 * 12 * 12 and scores.max() == scores[64]
    assert K.pick_index([5, 7, 7, 7, 5]) == 0 and K.pick_index([7, 5, 5, 5, 7]) == -2 and K.pick_index([1, 7, 5, 7, 1]) == -1
    assert K.pick_index([0, 0, 0, 0, 9]) == 2 and R.pick_brute([7, 5, 5, 5, 7]) == -2 and R.pick_brute([1, 7, 5, 7, 1]) == -1


def test_validation():
    page = R.random_grey(8, 9, seed=6)
    for bad in (dict(threshold=-2), dict(threshold=255), dict(polarity=-1), dict(polarity=3), dict(steps=-1), dict(steps=65), dict(steps=2.5),
                dict(slope_step=0), dict(slope_step=1025), dict(steps=17, slope_step=1024), dict(steps=64, slope_step=257), dict(fill=-2),
                dict(fill=256), dict(steps="many")):
        with pytest.raises(ValueError):
            K.check_params(**bad)
        with pytest.raises(ValueError):
            K.deskew_host(page, **bad)
    assert K.check_params() == dict(threshold=-1, polarity=0, steps=48, slope_step=256, fill=-1) == K.DEFAULTS
    assert K.check_params(steps=16, slope_step=1024)["steps"] == 16 and K.check_params(steps=64, slope_step=256, fill=255)["fill"] == 255
    for bad in (page.astype(np.int32), page[0], np.zeros((0, 4), np.uint8), np.zeros((1, 4097), np.uint8), np.zeros((4097, 1), np.uint8)):
        with pytest.raises(ValueError):
            K.estimate_skew_host(bad)
        with pytest.raises(ValueError):
            K.rotate_host(bad, 0)
    for bad in (dict(index=65), dict(index=-65), dict(index=1.5), dict(index=17, slope_step=1024), dict(index=0, fill=300)):
        with pytest.raises(ValueError):
            K.rotate_host(page, **bad)
    for bad in (dict(threshold=127), dict(polarity=1)):                      # adaptive decides what is ink
        with pytest.raises(ValueError):
            K.deskew_host(page, adaptive=True, **bad)
    with pytest.raises(ValueError):
        K.deskew_host(page, adaptive=dict(window=3))


@pytest.mark.parametrize("shaded", [False, True], ids=["flat", "shaded"])
def test_skewed_page_reads_in_order_after_the_deskew(shaded):
    """4 lines of 7 words at nine slopes: the estimate is the nearest k / 256, and on the deskewed page the unchanged detector finds the 28
    drawn rectangles, within 1 pixel, in reading order; on the raw page at the five steeper slopes the reading order is not the drawn one."""
    adaptive = dict(radius=15) if shaded else None
    for slope, want in zip(R.SLOPES, R.INDICES):
        page, rects = R.skewed_page(slope, shaded)
        assert page.shape == R.SKEW_SHAPE and len(rects) == 28
        flat, index = K.deskew_host(page, adaptive=adaptive)
        assert index == want == K.estimate_skew_host(page, adaptive=adaptive)[0], "slope %g" % slope
        assert np.array_equal(flat, K.rotate_host(page, index))
        got, info = D.detect_words_host(flat, gap_x=8, adaptive=adaptive)
        assert len(got) == 28, "slope %g: %d boxes" % (slope, len(got))
        dev = int(np.abs(got[D.reading_order(got)][:, :4] - rects).max())
        print("slope %g: index %d, deviation %d" % (slope, index, dev))
        assert dev <= (0 if slope == 0 else 1), "slope %g: a box %d pixels from the drawn one" % (slope, dev)
        if slope in R.UNREADABLE:
            raw, _ = D.detect_words_host(page, gap_x=8, adaptive=adaptive)
            assert len(raw) == 28                                          # the detector still finds every word on the raw page ...
            # ... but not line by line: the drawn word of a raw box is the one whose skewed centre the box holds
            th = np.arctan(slope)
            cr, cc = (rects[:, 0] + rects[:, 1] - 1) / 2.0 - 149.5, (rects[:, 2] + rects[:, 3] - 1) / 2.0 - 319.5
            pr, pc = 149.5 + np.cos(th) * cr + np.sin(th) * cc, 319.5 - np.sin(th) * cr + np.cos(th) * cc
            order = [int(np.flatnonzero((raw[k, 0] <= pr) & (pr < raw[k, 1]) & (raw[k, 2] <= pc) & (pc < raw[k, 3]))[0]) for k in D.reading_order(raw)]
            assert sorted(order) == list(range(28)) and order != list(range(28)), "slope %g" % slope


def test_source_list_and_flags():
    assert "deskew.hip" in native.SOURCES and os.path.exists(os.path.join(native.CSRC, "deskew.hip"))
    assert os.path.exists(os.path.join(native.CSRC, "otsu.h"))
    decl = native.parse_header()
    assert [len(decl[n][1]) for n in ("crnn_deskew_workspace_bytes", "crnn_deskew_estimate", "crnn_rotate_pages")] == [3, 11, 10]
    assert (K.STRIPS, K.BAND_R) == (4, 192) and K.BAND_R + 16 * K.STRIPS == 256      # one bin of a workgroup's band per lane
    sys.path.insert(0, PKG)
    import predict as cli
    import utils as U
    assert U.Deskewer is K.Deskewer and U.deskew_host is K.deskew_host and U.estimate_skew_host is K.estimate_skew_host
    assert U.rotate_host is K.rotate_host
    base = ["--model_path", "m", "--image_path", "i"]
    args = cli.parse_args(base + ["--detect", "--deskew", "--deskew_steps", "32", "--deskew_slope_step", "128"])
    assert cli.deskew_params(args) == dict(steps=32, slope_step=128)
    assert cli.deskew_params(cli.parse_args(base + ["--detect", "--deskew"])) == {}
    assert cli.deskew_params(cli.parse_args(base + ["--detect"])) is None
    args = cli.parse_args(base + ["--detect", "--deskew", "--detect_adaptive", "7"])
    assert cli.deskew_params(args) == dict(adaptive=dict(radius=7))
    assert cli.deskew_params(cli.parse_args(base + ["--detect", "--deskew", "--detect_threshold", "99"])) == dict(threshold=99)
    for bad in (["--deskew"], ["--deskew", "--deskew_steps", "8"], ["--detect", "--deskew_steps", "8"], ["--detect", "--deskew_slope_step", "8"],
                ["--detect", "--deskew", "--deskew_steps", "65"], ["--detect", "--deskew", "--deskew_slope_step", "0"],
                ["--detect", "--deskew", "--deskew_steps", "64", "--deskew_slope_step", "512"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert "--deskew_steps" in cli.build_parser().format_help()
