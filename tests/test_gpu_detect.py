"""-m gpu tests of word detection on the device (csrc/detect.hip, crnn_mi355x/detect.py).  Every case calls crnn_detect_words twice on outputs
pre-filled with a sentinel and a poisoned workspace, asserts that the two calls agree bit for bit, and that both equal detect_words_host (pinned
to scipy's labelling in tests/test_detect_cpu.py) in rects, ink counts and all four info words.  Everything is integer or fixed-order float64,
so every comparison is exact equality.  Shapes are the smallest at which the kernels take every path: one-pixel, one-row and one-column pages,
pages of several tiles that end off the tile grid, features placed on tile borders and corners (detect.TILE_R x detect.TILE_C)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import detect as D
from crnn_mi355x.pages import PAGE_DTYPE
from gpu_util import L, P, S, ok, host, sentinel_arena
import detect_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
T_R, T_C = D.TILE_R, D.TILE_C
SENTINELS = (77, -9)


def _call(arena_dev, arena_bytes, table, table_dev, n, prm, cap, fill, ws_bytes=None, ws_offset=0, null=None):
    """One call on outputs filled with `fill` -> (code, rects, info)."""
    rows = max(n, 1)
    rects = torch.full((rows, cap, 5), fill, dtype=torch.int32, device="cuda")
    info = torch.full((rows, 4), fill, dtype=torch.int32, device="cuda")
    need = L().crnn_detect_workspace_bytes(table.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(prm))
    nbytes = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(need, 16) // 4 + 8,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")   # the caller owes no zeroing
    args = dict(arena=ctypes.c_void_p(arena_dev.data_ptr()), pages=table.ctypes.data_as(ctypes.c_void_p), pages_dev=P(table_dev),
                prm=ctypes.byref(prm), rects=P(rects), info=P(info), ws=ctypes.c_void_p(ws.data_ptr() + ws_offset))
    if null:
        args[null] = ctypes.c_void_p(0)
    code = L().crnn_detect_words(args["arena"], arena_bytes, args["pages"], args["pages_dev"], n, args["prm"], args["rects"], args["info"],
                                 args["ws"], nbytes, S())
    torch.cuda.synchronize()
    return code, host(rects), host(info)


def _detect(pages, strides=None, cap=64, **params):
    """Two calls -> (rects (P, cap, 5), info (P, 4)), equal between the calls and equal to detect_words_host page by page."""
    p = dict(R.PLAIN, **params)
    prm = D.crnn_detect_params(cap=cap, **p)
    arena, table, _ = sentinel_arena(pages, strides)
    arena_dev, table_dev = torch.from_numpy(arena).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    outs = []
    for fill in SENTINELS:
        code, rects, info = _call(arena_dev, arena.size, table, table_dev, len(pages), prm, cap, fill)
        assert code == 0, "crnn_detect_words returned %d" % code
        outs.append((rects, info))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "two calls disagree"
    rects, info = outs[0]
    for k, pg in enumerate(pages):
        want, winfo = D.detect_words_host(pg, cap=cap, **p)
        assert info[k].tolist() == winfo.tolist(), "page %d (%s): info %s, host %s" % (k, pg.shape, info[k].tolist(), winfo.tolist())
        kept = int(winfo[1])
        assert np.array_equal(rects[k, :kept], want), "page %d (%s): boxes differ from the host's" % (k, pg.shape)
        assert (rects[k, kept:] == -1).all(), "page %d: rows past kept must hold -1" % k
    return rects, info


def _found(pages, **params):
    return _detect(pages, **params)[1][:, 0].tolist()


# ---- 1. random pages --------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 4 * 64 + 1), (4 * 64 + 1, 1), (3 * T_R + 5, 2 * T_C + 1)]


@pytest.mark.parametrize("gaps", R.GAPS)
def test_random_pages_equal_the_host(gaps):
    """Every size at every density, sixteen pages in one arena; with the fixed threshold and with Otsu and the automatic polarity."""
    pages = [R.random_page(r, c, d, seed=7 * k + gaps[0]) for k, ((r, c), d) in enumerate((s, d) for s in SIZES for d in R.DENSITIES)]
    _, info = _detect(pages, cap=4096, gap_x=gaps[0], gap_y=gaps[1])
    assert info[:, 0].max() > (64 if gaps == (0, 0) else 0)  # unsmeared, the big sparse page holds many components
    _detect(pages, cap=4096, gap_x=gaps[0], gap_y=gaps[1], threshold=-1, polarity=0)
    _detect(pages[12:], cap=4096, gap_x=gaps[0], gap_y=gaps[1], polarity=2, min_w=2, min_h=2, min_ink=3)


def test_pages_of_different_sizes_a_row_stride_and_a_constant_page():
    pages = [R.random_page(T_R + 3, T_C + 9, 0.3, seed=1), R.random_page(2 * T_R + 1, 37, 0.3, seed=2), np.full((9, 70), 131, np.uint8)]
    for thr in (127, -1):
        _, info = _detect(pages, strides=[T_C + 9, 64, 70], cap=1024, gap_x=1, gap_y=1, threshold=thr, polarity=0)
        assert info[2].tolist() == ([0, 0, -1, 1] if thr < 0 else [0, 0, 127, 1])
    # a constant dark page under a fixed threshold and dark ink is one box: the whole page
    rects, info = _detect([np.full((T_R + 1, T_C + 1), 5, np.uint8)], gap_x=3, gap_y=3)
    assert info[0].tolist() == [1, 1, 127, 1] and rects[0, 0].tolist() == [0, T_R + 1, 0, T_C + 1, (T_R + 1) * (T_C + 1)]


# ---- 2. equivalence chains, corners ----------------------------------------------------------------------------------------------------------------
def test_chains_across_every_tile_border():
    rows, cols = 3 * T_R, 3 * T_C
    pages = [R.from_mask(m) for m in (R.snake(rows, cols), R.comb(rows, cols), R.comb(rows, cols, spine=False), R.snake(rows, cols).T.copy())]
    assert _found(pages, cap=256) == [1, 1, cols // 2, 1]


def test_corners():
    def page(at):
        return R.from_mask(R.dots(2 * T_R, 2 * T_C, at))
    pages = [page([(T_R - 1, T_C - 1), (T_R, T_C)]), page([(T_R - 1, T_C), (T_R, T_C - 1)]), page([(T_R - 1, T_C - 1), (T_R + 1, T_C + 1)]),
             page([(T_R - 1, T_C - 1), (T_R - 1, T_C + 1)]), page([(T_R - 1, T_C - 1), (T_R, T_C - 1)]), page([(T_R, T_C - 1), (T_R, T_C)])]
    assert _found(pages) == [1, 1, 2, 2, 1, 1]


# ---- 3. smears across a tile border: the halo ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 5, 64])
def test_horizontal_and_vertical_smears_across_a_border(gap):
    a = gap // 2
    b = gap - a

    def pair(first, second, vertical):
        m = R.dots(2 * T_R, 3 * T_C, [(7, first), (7, second)])
        return R.from_mask(m.T.copy() if vertical else m)
    left = T_C - 1 - a                                       # ink at columns T_C - 1 - a and T_C + b: a + b clear pixels between
    pages = [pair(left, T_C + b, False), pair(left, T_C + b + 1, False), pair(2 * T_C - 1 - a, 2 * T_C + b, False)]
    assert _found(pages, gap_x=gap) == [1, 2, 1]
    assert _found(pages, gap_x=gap - 1) == [2, 2, 2]
    if gap <= 16:
        pages = [pair(T_R - 1 - a, T_R + b, True), pair(T_R - 1 - a, T_R + b + 1, True)]
        assert _found(pages, gap_y=gap) == [1, 2]
        assert _found(pages, gap_y=gap - 1, gap_x=64) == [2, 2]


def test_vertical_smear_of_16_rows_across_a_border():
    pages = [R.from_mask(R.dots(3 * T_R, T_C + 2, [(T_R - 9, c), (T_R + 8, c)])) for c in (0, T_C - 1, T_C, T_C + 1)]
    pages.append(R.from_mask(R.dots(3 * T_R, T_C + 2, [(T_R - 9, 5), (T_R + 9, 5)])))
    assert _found(pages, gap_y=16) == [1, 1, 1, 1, 2]


def test_runs_that_touch_the_page_edge_are_not_filled():
    m = R.dots(T_R + 4, T_C + 4, [(0, 3), (2, T_C), (T_R + 1, 0), (T_R + 1, T_C + 2)])
    rects, info = _detect([R.from_mask(m)], gap_x=64, gap_y=16)
    assert info[0, 0] == 4 and rects[0, :4, :4].tolist() == [[0, 1, 3, 4], [2, 3, T_C, T_C + 1], [T_R + 1, T_R + 2, 0, 1],
                                                              [T_R + 1, T_R + 2, T_C + 2, T_C + 3]]
    # ... while the run between two of them is: the last two join over T_C + 1 clear pixels only when gap_x reaches that
    assert _found([R.from_mask(R.dots(3, T_C + 4, [(1, 0), (1, T_C + 2)]))], gap_x=64) == [2]
    assert _found([R.from_mask(R.dots(3, 70, [(1, 0), (1, 65)]))], gap_x=64) == [1]


def test_the_horizontal_smear_comes_first():
    """An L shape: the horizontal smear makes the pixel that the vertical smear then reaches.  The other order leaves two components."""
    def shape(r, c):
        return R.from_mask(R.dots(3 * T_R, 3 * T_C, [(r - 2, c), (r + 2, c - 2), (r + 2, c + 2)]))
    # the filled row in the tile below (a halo row of the tile above, whose own smear needs the column halo), in the same tile, and off the borders
    pages = [shape(T_R - 1, T_C), shape(T_R, T_C), shape(T_R + 7, T_C + 9), shape(2 * T_R - 2, 2 * T_C - 1)]
    for pg in pages:
        ink = pg <= 127
        assert len(D.components(D.smear_rows(D.smear_rows(ink.T, 3).T, 3), ink)) == 2       # vertical first: two
    rects, info = _detect(pages, gap_x=3, gap_y=3)
    assert info[:, 0].tolist() == [1, 1, 1, 1] and rects[:, 0, 4].tolist() == [3, 3, 3, 3]  # ink counts the original pixels only


# ---- 4. cap and filter ------------------------------------------------------------------------------------------------------------------------------
def test_cap_keeps_the_first_in_index_order():
    at = [(3 * (k // 8) + (k % 2), 17 * (k % 8) + 5) for k in range(40)]          # 40 isolated pixels over three tile columns, both row parities
    page = R.from_mask(R.dots(15, 2 * T_C + 9, at))
    rects, info = _detect([page], cap=7)
    first = sorted(at)[:7]
    assert info[0].tolist() == [40, 7, 127, 1] and rects[0, :, 0].tolist() == [r for r, _ in first] and rects[0, :, 2].tolist() == [c for _, c in first]
    rects, info = _detect([page], cap=40)
    assert info[0].tolist() == [40, 40, 127, 1]
    rects, info = _detect([page, page], cap=41)
    assert (rects[:, 40] == -1).all()


def test_filter_bounds_at_equality_and_past_it():
    m = np.zeros((T_R + 8, T_C + 8), bool)
    m[T_R - 1:T_R + 2, T_C - 3:T_C + 3] = True                                      # 3 x 6 = 18 ink pixels over a tile corner
    m[1, 1] = True                                                                  # and a pixel the lower bounds drop
    page = R.from_mask(m)
    assert _found([page]) == [2]
    for key, at, past in (("min_w", 6, 7), ("min_h", 3, 4), ("min_ink", 18, 19)):
        assert _found([page], **{key: at}) == [1] and _found([page], **{key: past}) == [0]
    for key, at, past in (("max_w", 6, 5), ("max_h", 3, 2)):
        assert _found([page], **{key: at}) == [2] and _found([page], **{key: past}) == [1]


# ---- 5. the refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    pages = [R.random_page(T_R + 3, T_C + 9, 0.3, seed=1), R.random_page(5, 7, 0.3, seed=2)]
    arena, table, _ = sentinel_arena(pages)
    arena_dev, table_dev = torch.from_numpy(arena).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    good = dict(R.PLAIN, cap=8)

    def refused(code, table=table, n=2, arena_bytes=arena.size, **kw):
        prm = D.crnn_detect_params(**dict(good, **kw.pop("prm", {})))
        got, rects, info = _call(arena_dev, arena_bytes, table, table_dev, n, prm, 8, 77, **kw)
        assert got == code, "expected %d, got %d" % (code, got)
        assert (rects == 77).all() and (info == 77).all()

    def edited(k, **fields):
        t = table.copy()
        for name, v in fields.items():
            t[name][k] = v
        return t
    assert _call(arena_dev, arena.size, table, table_dev, 2, D.crnn_detect_params(**good), 8, 77)[0] == 0
    for name in ("arena", "pages", "pages_dev", "prm", "rects", "info", "ws"):
        refused(-2, null=name)
    refused(-2, n=-1)
    refused(0, n=0)                                                                  # P == 0 launches nothing
    refused(-2, table=edited(1, page_off=arena.size))                               # a page outside the arena
    refused(-2, table=edited(1, page_off=-16))
    refused(-2, arena_bytes=int(table["page_off"][1]) + 5 * 7 - 1)
    refused(-2, table=edited(0, stride=T_C + 8))                                    # stride < cols
    refused(-2, table=edited(0, rows=0))
    refused(-2, table=edited(1, cols=0))
    for bad in (dict(threshold=255), dict(threshold=-2), dict(polarity=3), dict(polarity=-1), dict(gap_x=65), dict(gap_x=-1), dict(gap_y=17),
                dict(gap_y=-1), dict(min_w=-1), dict(min_h=-1), dict(min_ink=-1), dict(max_w=-1), dict(max_h=-1), dict(cap=0)):
        refused(-2, prm=bad)
    need = L().crnn_detect_workspace_bytes(table.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(D.crnn_detect_params(**good)))
    assert need >= 4 * sum(pg.size for pg in pages)
    refused(-2, ws_bytes=need - 1)                                                   # a short workspace
    refused(-2, ws_offset=4)                                                         # a misaligned one
    # -3: a page above 4096 in either direction, more than 2^31 pixels in one call (the pages of a table may share bytes)
    wide = np.zeros(1, PAGE_DTYPE); wide[0] = (0, 1, 4097, 4097)
    refused(-3, table=wide, n=1)
    tall = np.zeros(1, PAGE_DTYPE); tall[0] = (0, 4097, 1, 1)
    refused(-3, table=tall, n=1)
    big = torch.zeros(4096 * 4096, dtype=torch.uint8, device="cuda")
    many = np.zeros(129, PAGE_DTYPE); many[:] = (0, 4096, 4096, 4096)
    many_dev = torch.from_numpy(many.view(np.uint8)).cuda()
    prm = D.crnn_detect_params(**good)
    assert L().crnn_detect_workspace_bytes(many.ctypes.data_as(ctypes.c_void_p), 129, ctypes.byref(prm)) == 0
    code, rects, info = _call(big, big.numel(), many, many_dev, 129, prm, 8, 77)
    assert code == -3 and (rects == 77).all() and (info == 77).all()


# ---- 6. the surface --------------------------------------------------------------------------------------------------------------------------------------
def test_rendered_page_gives_the_eleven_words():
    page, truth = R.fixture()
    rects, info = _detect([page], polarity=0, gap_x=6)
    assert info[0].tolist() == [11, 11, 127, 1]
    got = rects[0, :11]
    assert np.array_equal(got[D.reading_order(got)][:, :4], truth)
    det = U.WordDetector(threshold=127, gap_x=6, gap_y=0)
    assert det.boxes([page]) == [[(None, int(b[0]), int(b[2]), int(b[1]), int(b[3])) for b in truth]]
    assert _found([page], polarity=0, gap_x=13) == [3] and _found([page], polarity=0, gap_x=1) == [22]


def test_word_detector_warns_once_when_a_page_overflows_its_cap():
    page, _ = R.fixture()
    det = U.WordDetector(threshold=127, gap_x=6, cap=4)
    with pytest.warns(UserWarning, match="page 1 holds 11 boxes"):
        out = det.detect([np.full((4, 4), 9, np.uint8), page])
    assert out[0][1].tolist() == [0, 0, 127, 0] and out[1][1].tolist() == [11, 4, 127, 1] and out[1][0].shape == (4, 5)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        det.detect([page])                                                           # once per detector


def test_detector_and_ingest_share_one_upload():
    page, truth = R.fixture()
    noise = R.random_page(90, 200, 0.02, seed=5)
    pages = [page, noise]
    ing = U.DeviceIngest((100, 32, 1))
    det = U.WordDetector(threshold=127, gap_x=6, gap_y=2)
    arena = ing.upload(pages)
    boxes = det.boxes(None, arena=arena)
    assert len(boxes[0]) == 11 and len(boxes[1]) >= 3
    assert boxes == [D.to_boxes(D.detect_words_host(pg, threshold=127, gap_x=6, gap_y=2)[0]) for pg in pages]
    index = [k for k, bl in enumerate(boxes) for _ in bl]
    rects = [U.box_slices(b, pages[k].shape) for k, bl in enumerate(boxes) for b in bl]
    shared = ing.crops(None, index, rects, ing.plan(rects), arena=arena)
    again = ing.crops(None, index[:5], rects[:5], ing.plan(rects[:5]), batch=8, arena=arena)      # the arena outlives a launch
    plain, words = ing.pages(pages, boxes)
    assert shared.shape == (len(index), 100, 32, 1) and torch.equal(shared, plain) and words == ["-"] * len(index)
    assert torch.equal(again[:5], plain[:5]) and not again[5:].any()


def test_predict_cli_detects_on_the_device_and_on_the_host(tmp_path, capsys):
    """predict.py --detect --device_ingest and predict.py --detect write identical prediction.csv files, one row per box of detect_words_host."""
    from PIL import Image
    page, _ = R.fixture()
    pdir = tmp_path / "pages"
    os.makedirs(pdir)
    pages = {"a_fixture.png": page, "b_noise.png": R.random_page(60, 150, 0.03, seed=11), "c_blank.png": np.full((20, 30), 240, np.uint8)}
    for name, pg in pages.items():
        Image.fromarray(pg).save(str(pdir / name))
    m = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    U.save_model_json(m, str(tmp_path / "models"), "m1")
    m.save_weights(str(mdir / "final_weights.h5"))
    sys.path.insert(0, PKG)
    import predict as predict_cli
    import pandas as pd
    base = ["--model_path", str(mdir), "--image_path", str(pdir), "--batch_size", "8", "--G", "0", "--detect", "--detect_gap_x", "6",
            "--detect_gap_y", "1", "--detect_min_w", "2", "--detect_min_h", "2", "--detect_min_ink", "2", "--detect_threshold", "127"]
    seen = []
    for flags in ([], ["--device_ingest"]):
        res = tmp_path / ("res%d" % len(flags))
        os.makedirs(res)
        capsys.readouterr()
        predict_cli.main(base + ["--result_path", str(res)] + flags)
        out = capsys.readouterr().out
        assert "1 page(s) without a word box left out: c_blank.png" in out
        seen.append(open(res / "prediction.csv").read())
    assert seen[0] == seen[1]
    table = pd.read_csv(tmp_path / "res0" / "prediction.csv")
    want = []
    for name in ("a_fixture.png", "b_noise.png"):
        rects, _ = D.detect_words_host(U.read_img(str(pdir / name)), threshold=127, gap_x=6, gap_y=1, min_w=2, min_h=2, min_ink=2)
        want += [(str(pdir / name), int(r[0]), int(r[2]), int(r[1]), int(r[3])) for r in rects[D.reading_order(rects)]]
    assert len(want) > 11 and list(zip(table["fname"], table["r0"], table["c0"], table["r1"], table["c1"])) == want
