"""CPU tests (no GPU) of the page-arena contract: csrc/pages.h through the entry points that validate a page table, and crnn_mi355x/pages.py.

The entry points check their arguments on the host before anything is launched (as tests/test_ingest_cpu.py shows for crnn_ingest_crops), so
a fake non-null integer stands for every device pointer and no pointer is ever followed.  One table of faulty page entries and arena sizes is
run against crnn_detect_workspace_bytes, crnn_detect_words, crnn_binarize_pages, crnn_deskew_workspace_bytes, crnn_deskew_estimate,
crnn_rotate_pages and, for its page fields, crnn_ingest_crops.  The expected codes were recorded from the library as it was BEFORE the checks
moved into csrc/pages.h (each entry point then had its own copy of them); they are not derived from the header.  A case is run only against
the entry points that refuse it: one that accepts it would launch on the fake pointers.  For that reason the table cannot show that
crnn_ingest_crops accepts a page above 4096 (it has no such limit): the 4097-row entries here do not fit the arena, which is what it refuses."""
import ctypes

import numpy as np
import pytest

from crnn_mi355x import binarize as B, deskew as K, detect as D, ingest as I, native, pages as PG

ARG, UNSUPPORTED = -2, -3
ARENA_P, OUT_P, FAKE = 1 << 20, 1 << 24, ctypes.c_void_p(1 << 22)      # stand for device pointers
SHAPES = [(20, 70), (5, 7)]                                            # page 1 begins at byte 1408, the arena holds 1456 bytes
OFF1, NBYTES = 1408, 1456
ZERO, SIZE = "0", ">0"                                                 # what a *_workspace_bytes call returns


def _table(n=None, **edits):
    """The table of SHAPES packed back to back (or n one-pixel pages at offset 0), entry k edited by edits['e<k>'] = dict(field=value)."""
    if n is None:
        t = PG.page_table([np.zeros(s, np.uint8) for s in SHAPES], [0, OFF1])
    else:
        t = np.zeros(n, PG.PAGE_DTYPE)
        t[:] = (0, 1, 1, 1)
    for key, fields in edits.items():
        for name, v in fields.items():
            t[name][int(key[1:])] = v
    return t


# name -> (table, arena_bytes, out_bytes, out pointer, {entry point: expected}); an entry point that is absent is not run on the case
ALL_ARG = dict(dws=ZERO, det=ARG, bin=ARG, kws=ZERO, est=ARG, rot=ARG, ing=ARG)
OVER = dict(dws=ZERO, det=UNSUPPORTED, bin=ARG, kws=ZERO, est=UNSUPPORTED, rot=UNSUPPORTED, ing=ARG)
NO_FIT = dict(dws=SIZE, det=ARG, bin=ARG, kws=SIZE, est=ARG, rot=ARG, ing=ARG)      # the workspace sizes do not look at the arena
MANY = dict(dws=ZERO, det=UNSUPPORTED, bin=UNSUPPORTED, kws=ZERO, est=UNSUPPORTED, rot=UNSUPPORTED)
CASES = {
    "rows of 0": (_table(e1=dict(rows=0)), NBYTES, NBYTES, OUT_P, ALL_ARG),
    "cols of 0": (_table(e0=dict(cols=0)), NBYTES, NBYTES, OUT_P, ALL_ARG),
    "rows of 4097": (_table(e0=dict(rows=4097)), NBYTES, NBYTES, OUT_P, OVER),
    "cols of 4097": (_table(e1=dict(cols=4097, stride=4097)), NBYTES, NBYTES, OUT_P, OVER),
    "stride below cols": (_table(e0=dict(stride=69)), NBYTES, NBYTES, OUT_P, ALL_ARG),
    "negative offset": (_table(e1=dict(page_off=-16)), NBYTES, NBYTES, OUT_P, ALL_ARG),
    "offset equal to the arena size": (_table(e1=dict(page_off=NBYTES)), NBYTES, NBYTES, OUT_P, NO_FIT),
    "extent one byte past the input arena": (_table(), OFF1 + 5 * 7 - 1, NBYTES, OUT_P, NO_FIT),
    "extent one byte past the output arena": (_table(), NBYTES, OFF1 + 5 * 7 - 1, OUT_P, dict(bin=ARG, rot=ARG)),
    "overlap: the output begins on the input's last byte": (_table(), NBYTES, NBYTES, ARENA_P + NBYTES - 1, dict(bin=ARG, rot=ARG)),
    "overlap: the output ends on the input's first byte": (_table(), NBYTES, NBYTES, ARENA_P - NBYTES + 1, dict(bin=ARG, rot=ARG)),
    "overlap: the same range": (_table(), NBYTES, NBYTES, ARENA_P, dict(bin=ARG, rot=ARG)),
    "65536 pages": (_table(65536), 16, 16, OUT_P, MANY),
    "65536 pages, the last one faulty: the table is judged first": (
        _table(65536, e65535=dict(rows=0)), 16, 16, OUT_P, dict(MANY, det=ARG, bin=ARG, est=ARG, rot=ARG)),
    "one entry, two faults: stride below cols and above 4096": (_table(e1=dict(cols=4097)), NBYTES, NBYTES, OUT_P, ALL_ARG),
    "one entry, two faults: above 4096 and outside the arena": (
        _table(e1=dict(rows=4097, page_off=NBYTES)), NBYTES, NBYTES, OUT_P, OVER),
    "two entries: above 4096, then rows of 0": (_table(e0=dict(rows=4097), e1=dict(rows=0)), NBYTES, NBYTES, OUT_P, OVER),
    "two entries: rows of 0, then above 4096": (_table(e0=dict(rows=0), e1=dict(rows=4097)), NBYTES, NBYTES, OUT_P, ALL_ARG),
    "two entries: above 4096, then outside the arena": (_table(e0=dict(cols=4097, stride=4097), e1=dict(page_off=NBYTES)), NBYTES, NBYTES, OUT_P, OVER),
    "two entries: outside the arena, then above 4096": (
        _table(e0=dict(page_off=NBYTES), e1=dict(cols=4097, stride=4097)), NBYTES, NBYTES, OUT_P, dict(NO_FIT, dws=ZERO, kws=ZERO)),
}


def _crop_items(table):
    """One crnn_crop_item per table entry: the one-pixel box at the page's corner, valid in everything but the entry's own page fields."""
    n = len(table)
    up, size, place = I.plan_crop(1, 1, (100, 32, 1))
    plans = tuple(np.full(n, v) for v in (up,) + size + place)
    items = I.build_table([np.zeros((1, 1), np.uint8)] * n, [0] * n, list(range(n)), [(0, 1, 0, 1)] * n, plans, (100, 32, 1))
    for name in ("page_off", "rows", "cols", "stride"):
        items[name] = table[name]
    return items


def _run(which, table, arena_bytes, out_bytes, out_p):
    L, n = native.lib(), len(table)
    host = table.ctypes.data_as(ctypes.c_void_p)
    arena, out = ctypes.c_void_p(ARENA_P), ctypes.c_void_p(out_p)
    det, bin_, dsk = D.crnn_detect_params(**D.DEFAULTS), B.crnn_binarize_params(**B.DEFAULTS), K.crnn_deskew_params(**K.DEFAULTS)
    if which == "dws":
        return L.crnn_detect_workspace_bytes(host, n, ctypes.byref(det))
    if which == "det":
        return L.crnn_detect_words(arena, arena_bytes, host, FAKE, n, ctypes.byref(det), FAKE, FAKE, FAKE, 1 << 40, None)
    if which == "bin":
        return L.crnn_binarize_pages(arena, arena_bytes, host, FAKE, n, ctypes.byref(bin_), out, out_bytes, None)
    if which == "kws":
        return L.crnn_deskew_workspace_bytes(host, n, ctypes.byref(dsk))
    if which == "est":
        return L.crnn_deskew_estimate(arena, arena_bytes, host, FAKE, n, ctypes.byref(dsk), FAKE, FAKE, FAKE, 1 << 40, None)
    if which == "rot":
        return L.crnn_rotate_pages(arena, arena_bytes, host, FAKE, n, FAKE, ctypes.byref(dsk), out, out_bytes, None)
    items = _crop_items(table)
    return L.crnn_ingest_crops(arena, arena_bytes, items.ctypes.data_as(ctypes.c_void_p), FAKE, n, n, 100, 32, FAKE, FAKE, None, None)


@pytest.mark.parametrize("name", list(CASES))
def test_faulty_page_tables_are_refused_with_the_recorded_codes(name):
    table, arena_bytes, out_bytes, out_p, expected = CASES[name]
    for which, want in expected.items():
        got = _run(which, table, arena_bytes, out_bytes, out_p)
        if want in (ZERO, SIZE):
            assert (got == 0) == (want == ZERO), "%s, %s: returned %d, expected %s" % (name, which, got, want)
        else:
            assert got == want, "%s, %s: returned %d, expected %d" % (name, which, got, want)


def test_every_fault_of_the_list_meets_every_entry_point_that_judges_it():
    """The table above leaves an entry point out only where it has no output arena, or (crnn_ingest_crops) no page count limit."""
    for name, (_, _, _, _, expected) in CASES.items():
        missing = set(ALL_ARG) - set(expected)
        if "output" in name or "overlap" in name:
            assert missing == {"dws", "det", "kws", "est", "ing"}, name
        else:
            assert missing <= {"ing"} and (not missing or "65536" in name), name


# ---- crnn_mi355x/pages.py ---------------------------------------------------------------------------------------------------------------------
LIMITED = "a page is a non-empty (H, W) uint8 array of at most 4096 x 4096, not %s %s"      # detect.ink_mask, binarize.sauvola_host, deskew
UNLIMITED = "a page is a non-empty (H, W) uint8 array, not %s %s"                           # ingest.arena_layout


def test_check_page_accepts_and_refuses_what_the_four_copies_did():
    good = [np.zeros((1, 1), np.uint8), np.zeros((4096, 1), np.uint8), np.zeros((3, 4096), np.uint8), np.zeros((8, 8), np.uint8)[:, ::2]]
    for pg in good:
        assert PG.check_page(pg) is pg and PG.check_page(pg, None) is pg
    bad = [np.zeros((3, 3), np.float32), np.zeros((3, 3), np.int8), np.zeros((3,), np.uint8), np.zeros((2, 3, 1), np.uint8),
           np.zeros((0, 5), np.uint8), np.zeros((5, 0), np.uint8)]
    for pg in bad:
        for limit, text in ((PG.MAX_DIM, LIMITED), (None, UNLIMITED)):
            with pytest.raises(ValueError) as e:
                PG.check_page(pg, limit)
            assert str(e.value) == text % (pg.dtype, pg.shape)
    for pg in (np.zeros((4097, 1), np.uint8), np.zeros((1, 4097), np.uint8)):
        assert PG.check_page(pg, None) is pg                                       # the arena itself has no limit
        for call in (PG.check_page, D.ink_mask, B.sauvola_host, lambda p: K.rotate_host(p, 0), K.skew_scores_host):
            with pytest.raises(ValueError) as e:
                call(pg)
            assert str(e.value) == LIMITED % (pg.dtype, pg.shape)
    with pytest.raises(ValueError) as e:
        PG.arena_layout([np.zeros((3, 3), np.float32)])
    assert str(e.value) == UNLIMITED % ("float32", (3, 3))
    assert PG.arena_layout([np.zeros((4097, 3), np.uint8)]) == ([0], 12304)


def test_page_table_on_pages_with_gaps_between_them():
    shapes = [(37, 61), (5, 3), (1, 1), (64, 16), (3, 7)]                          # 2257 -> 2272, 15 -> 16, 1 -> 16, 1024 (no gap), 21
    pages = [np.zeros(s, np.uint8) for s in shapes]
    offs, total = PG.arena_layout(pages)
    assert offs == [0, 2272, 2288, 2304, 3328] and total == 3360
    old = np.zeros(len(pages), PG.PAGE_DTYPE)                                      # the table as detect.page_table built it
    for k, (pg, off) in enumerate(zip(pages, offs)):
        old[k] = (off, pg.shape[0], pg.shape[1], pg.shape[1])
    got = PG.page_table(pages, offs)
    assert got.dtype == PG.PAGE_DTYPE and got.tobytes() == old.tobytes()
    raw = (PG.crnn_page_item * len(got)).from_buffer_copy(got.tobytes())           # the bytes as the C side reads them
    assert [(it.page_off, it.rows, it.cols, it.stride) for it in raw] == [(o, r, c, c) for o, (r, c) in zip(offs, shapes)]
    assert ctypes.sizeof(PG.crnn_page_item) == PG.PAGE_DTYPE.itemsize == 24


def test_page_arena_builds_its_table_once_and_shares_it():
    import torch
    pages = [np.full(s, 7, np.uint8) for s in SHAPES]
    packed, offs = PG.pack_arena(pages)
    arena = PG.PageArena(pages, offs, len(packed), None, torch.from_numpy(packed))         # (a host tensor stands for the device arena)
    table = arena.table
    assert arena.table is table and table.tobytes() == PG.page_table(pages, offs).tobytes()
    made = arena.blank()
    assert made is not arena and made.host is None and made.pages is arena.pages and made.offsets is arena.offsets and made.nbytes == arena.nbytes
    assert made.dev.dtype == torch.uint8 and made.dev.numel() == arena.nbytes and not made.dev.any() and made.dev.device == arena.dev.device
    assert made.table is table and made.blank().table is table
    dev = made.table_dev                                                           # made on first use, by whichever arena asks first
    assert arena.table_dev is dev and made.table_dev is dev and dev.numpy().tobytes() == table.tobytes()
    assert PG.PageArena([], [], 0, None, torch.zeros(1, dtype=torch.uint8)).blank().dev.numel() == 1
