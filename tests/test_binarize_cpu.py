"""Adaptive binarisation on the host (crnn_mi355x/binarize.py): sauvola_host against the brute-force restatement of tests/binarize_ref.py
(Python ints, math.isqrt), the properties of the rule, the validation, the shaded page that one global threshold cannot split -- the reason
for the feature -- and the source list and flags.  Everything is integer: every comparison is exact equality."""
import os
import sys

import numpy as np
import pytest

from crnn_mi355x import binarize as B, detect as D, native
import binarize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (37, 1), (23, 41), (40, 50)])
def test_host_equals_the_brute_force_rule(shape):
    page = R.random_grey(*shape, seed=shape[0] + shape[1])
    for radius in (1, 2, 5, 31):
        for k256 in (0, 51, 128, 255):
            for polarity in (1, 2):
                got = B.sauvola_host(page, radius, k256, polarity)
                assert got.dtype == np.uint8 and got.shape == page.shape and set(np.unique(got)) <= {0, 255}
                assert np.array_equal(got, R.sauvola_brute(page, radius, k256, polarity)), (shape, radius, k256, polarity)


@pytest.mark.parametrize("name", ["checkerboard", "half_page"])
def test_extremes_of_the_arithmetic(name):
    """0 / 255 over a full window at r = 31, k256 = 255: the largest D and the largest products (the brute force asserts they fit)."""
    page = getattr(R, name)(130, 130)
    got = B.sauvola_host(page, polarity=1, **R.EXTREME)
    assert np.array_equal(got, R.sauvola_brute(page, polarity=1, **R.EXTREME))
    assert (got == 0).any() and (got == 255).any()
    assert np.array_equal(B.sauvola_host(255 - page, polarity=2, **R.EXTREME), got)


def test_one_dark_pixel_on_a_white_page():
    page = R.one_dark_pixel(20, 30, (7, 11))
    for radius in (1, 5, 31):
        got = B.sauvola_host(page, radius=radius)
        assert np.array_equal(got, R.sauvola_brute(page, radius, 51, 1))
        assert got[7, 11] == 0 and (got == 0).sum() == 1
    assert (B.sauvola_host(page, radius=5, polarity=2) == 0).sum() > 1           # light ink: the white around the pixel stands out, the pixel does not
    assert B.sauvola_host(page, radius=5, polarity=2)[7, 11] == 255


def test_constant_pages_have_no_ink():
    for value in (0, 128, 255):
        for polarity in (1, 2):
            for k256 in (0, 51, 255):
                assert (B.sauvola_host(np.full((9, 13), value, np.uint8), 3, k256, polarity) == 255).all()


def test_k_zero_compares_with_the_window_mean():
    page = R.random_grey(19, 27, seed=4)
    v = page.astype(np.int64)
    want = np.zeros(page.shape, bool)
    for i in range(19):
        for j in range(27):
            w = v[max(0, i - 2):i + 3, max(0, j - 2):j + 3]
            want[i, j] = v[i, j] * w.size < w.sum()
    assert np.array_equal(B.sauvola_host(page, 2, 0, 1) == 0, want)


def test_light_ink_is_dark_ink_on_the_complement():
    page = R.random_grey(33, 29, seed=5)
    for radius, k256 in ((1, 0), (4, 51), (31, 255)):
        assert np.array_equal(B.sauvola_host(page, radius, k256, 2), B.sauvola_host(255 - page, radius, k256, 1))


def test_validation_and_the_float_k():
    page = R.random_grey(8, 9, seed=6)
    for bad in (dict(radius=0), dict(radius=32), dict(radius=2.5), dict(k256=-1), dict(k256=256), dict(polarity=0), dict(polarity=3),
                dict(k=1.0), dict(k=-0.1)):
        with pytest.raises(ValueError):
            B.sauvola_host(page, **bad)
    for bad in (page.astype(np.int32), page[0], np.zeros((0, 4), np.uint8), np.zeros((1, 4097), np.uint8), np.zeros((4097, 1), np.uint8)):
        with pytest.raises(ValueError):
            B.sauvola_host(bad)
    assert B.check_params(k=0.2) == dict(radius=15, k256=51, polarity=1) == B.check_params() == B.adaptive_params(True)
    assert np.array_equal(B.sauvola_host(page, 3, k=0.2), B.sauvola_host(page, 3, 51))
    assert B.adaptive_params(dict(radius=7)) == dict(radius=7, k256=51, polarity=1)
    for bad in (dict(window=3), 15, dict(radius=40)):
        with pytest.raises(ValueError):
            B.adaptive_params(bad)


def test_shaded_page_needs_the_adaptive_rule():
    """32 words under a brightness gradient: Otsu's one threshold does not find them (it finds one box: the dark half of the page), the
    adaptive rule finds exactly the drawn rectangles at every radius."""
    page, rects = R.shaded_page()
    assert page.shape == R.SHADED_SHAPE and len(rects) == 32
    plain, info = D.detect_words_host(page, gap_x=8)
    assert len(plain) != 32
    print("Otsu alone: %d box(es), info %s" % (len(plain), info.tolist()))
    for radius in R.SHADED_RADII:
        got, info = D.detect_words_host(page, gap_x=8, adaptive=dict(radius=radius))
        assert info.tolist() == [32, 32, 127, 1]
        assert np.array_equal(got[:, :4], rects), "radius %d" % radius
        binary = B.sauvola_host(page, radius=radius)
        assert got[:, 4].tolist() == [int((binary[a:b, c:d] == 0).sum()) for a, b, c, d in rects]     # ink counts binarised ink


def test_adaptive_goes_with_neither_threshold_nor_polarity():
    page, _ = R.shaded_page()
    for bad in (dict(threshold=127), dict(polarity=1), dict(polarity=2)):
        with pytest.raises(ValueError):
            D.detect_words_host(page, adaptive=True, **bad)
        with pytest.raises(ValueError):
            D.adaptive_setup(dict(radius=7), bad.get("threshold", -1), bad.get("polarity", 0))
    a, _ = D.detect_words_host(page, gap_x=8, adaptive=True)
    b, _ = D.detect_words_host(page, gap_x=8, adaptive=dict(B.DEFAULTS))
    assert np.array_equal(a, b)
    light, _ = D.detect_words_host(255 - page, gap_x=8, adaptive=dict(polarity=2))
    assert np.array_equal(light, a)
    assert D.adaptive_setup(None, 99, 2) == (None, 99, 2)                      # without it nothing changes


def test_source_list_and_flags():
    assert "binarize.hip" in native.SOURCES
    decl = native.parse_header()
    assert "crnn_binarize_pages" in decl and len(decl["crnn_binarize_pages"][1]) == 9
    assert (B.STRIP_C, B.BAND_R) == (192, 64) and B.STRIP_C + 2 * (B.MAX_RADIUS + 1) == 256
    sys.path.insert(0, PKG)
    import predict as cli
    import utils as U
    assert U.Binarizer is B.Binarizer and U.sauvola_host is B.sauvola_host
    base = ["--model_path", "m", "--image_path", "i"]
    args = cli.parse_args(base + ["--detect", "--detect_adaptive", "7", "--detect_adaptive_k", "0.3", "--detect_gap_x", "6"])
    assert cli.detect_params(args) == dict(gap_x=6, adaptive=dict(radius=7, k=0.3))
    assert cli.detect_params(cli.parse_args(base + ["--detect", "--detect_adaptive", "15"])) == dict(adaptive=dict(radius=15))
    for bad in (["--detect_adaptive", "7"], ["--detect_adaptive", "7", "--detect_adaptive_k", "0.2"], ["--detect", "--detect_adaptive_k", "0.2"],
                ["--detect", "--detect_adaptive", "32"], ["--detect", "--detect_adaptive", "0"], ["--detect", "--detect_adaptive", "7", "--detect_adaptive_k", "1.5"],
                ["--detect", "--detect_adaptive", "7", "--detect_threshold", "127"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert "grey" in cli.build_parser().format_help()
