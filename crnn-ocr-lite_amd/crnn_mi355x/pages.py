"""The page arena, stated once for the four stages that work on it (ingest, detect, binarize, deskew; for the library: csrc/pages.h).  Pages are
(H, W) uint8 arrays; an arena holds them back to back on 16-byte boundaries, each row-major without row padding, and a crnn_page_item table
(include/crnn_mi355x.h) says where each page lies.  `PageArena` is an arena on the device with its table; a stage reads one and, when it makes
pages, writes another of the same layout (`PageArena.blank`).  A leaf module: it imports nothing from the stages."""
import ctypes
import re

import numpy as np

from . import native

MAX_DIM = 4096                                               # rows and cols of a page the detector, the binarisation and the deskew take
_ARENA_ALIGN = 16


def header_int(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(native.HEADER).read())
    if m is None:
        raise RuntimeError("%s is not defined in %s" % (name, native.HEADER))
    return int(m.group(1))


class crnn_page_item(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_page_item."""
    _fields_ = [("page_off", ctypes.c_long), ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("stride", ctypes.c_int)]


PAGE_DTYPE = np.dtype([("page_off", np.dtype("l")), ("rows", np.intc), ("cols", np.intc), ("stride", np.intc)], align=True)
assert PAGE_DTYPE.itemsize == ctypes.sizeof(crnn_page_item)


def check_page(page, max_dim=MAX_DIM):
    """-> the page as an array; ValueError unless it is a non-empty (H, W) uint8 array of at most max_dim x max_dim (None: any size)."""
    page = np.asarray(page)
    if page.ndim != 2 or page.dtype != np.uint8 or page.size == 0 or (max_dim is not None and max(page.shape) > max_dim):
        limit = "" if max_dim is None else " of at most %d x %d" % (max_dim, max_dim)
        raise ValueError("a page is a non-empty (H, W) uint8 array%s, not %s %s" % (limit, page.dtype, page.shape))
    return page


def arena_layout(pages):
    """-> ([byte offset per page], arena size): pages back to back, each one row-major without row padding, on 16-byte boundaries."""
    offs, pos = [], 0
    for pg in pages:
        check_page(pg, None)
        offs.append(pos)
        pos += -(-pg.size // _ARENA_ALIGN) * _ARENA_ALIGN
    return offs, pos


def pack_arena(pages, out=None):
    """Copy the pages into one uint8 arena (a view of `out` when given) -> (arena, offsets)."""
    offs, total = arena_layout(pages)
    arena = np.zeros(total, np.uint8) if out is None else out[:total]
    for pg, o in zip(pages, offs):
        arena[o:o + pg.size].reshape(pg.shape)[...] = pg
    return arena, offs


def page_table(pages, offsets):
    """The crnn_page_item table of pages packed as pack_arena packs them."""
    t = np.zeros(len(pages), PAGE_DTYPE)
    for k, (pg, off) in enumerate(zip(pages, offsets)):
        t[k] = (off, pg.shape[0], pg.shape[1], pg.shape[1])
    return t


class PageArena:
    """Pages on the device: `dev` is the uint8 arena (pack_arena's layout), `pages` / `offsets` what it holds.  One upload serves the word
    detector (detect.WordDetector), the stages in front of it and any number of crop launches (DeviceIngest.crops(arena=...)); the
    page-locked source of the copy lives as long as the arena.  The arena owns its crnn_page_item table: `table` (host) is built once per
    layout, `table_dev` is copied to the arena's device on first use, and the arenas `blank` derives share both."""

    def __init__(self, pages, offsets, nbytes, host, dev, like=None):
        self.pages, self.offsets, self.nbytes, self.host, self.dev = pages, offsets, nbytes, host, dev
        self.table = page_table(pages, offsets) if like is None else like.table
        self._table_dev = [] if like is None else like._table_dev    # the one device copy of `table`, shared with the arenas blank() derives

    @property
    def table_dev(self):
        if not self._table_dev:
            import torch
            self._table_dev.append(torch.from_numpy(self.table.view(np.uint8)).to(self.dev.device))
        return self._table_dev[0]

    def blank(self):
        """-> a new zero-filled arena of this layout on this device (so its alignment bytes are zero); it shares both tables, `host` is None."""
        import torch
        return PageArena(self.pages, self.offsets, self.nbytes, None, torch.zeros(max(self.nbytes, 1), dtype=torch.uint8, device=self.dev.device),
                         like=self)


def upload_pages(pages, device):
    """list of (H, W) uint8 arrays -> PageArena on `device`: one page-locked buffer, one asynchronous copy on the current stream."""
    import torch
    pages = [np.ascontiguousarray(pg) for pg in pages]
    offs, nbytes = arena_layout(pages)
    device = torch.device(device)
    with torch.cuda.device(device):
        host = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        pack_arena(pages, out=host.numpy())
        dev = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        dev.copy_(host, non_blocking=True)
    return PageArena(pages, offs, nbytes, host, dev)


class StagingSlots:
    """Page-locked host buffers with their device twins, for the small tables a launch takes along (the ingest's arena and box table, the
    augmentation's items): take(nbytes) -> {"host", "dev", "np", "copied"} of the next slot, grown to a power of two of at least `floor`
    bytes.  A slot's host buffer is handed out again only after its previous copy has finished (the Engine.stage pattern): the caller records
    "copied" on the stream after its H->D copy.  Copy and kernel are ordered by the stream, so successive calls belong on one stream."""

    def __init__(self, device, slots=2, floor=1 << 20):
        import torch
        self.device, self.floor = device, int(floor)
        self._slots = [{"host": None, "dev": None, "copied": torch.cuda.Event()} for _ in range(slots)]
        self._next = 0

    def take(self, nbytes):
        import torch
        s = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        s["copied"].synchronize()                       # the previous H->D copy out of this slot's host buffer is done
        if s["host"] is None or s["host"].numel() < nbytes:
            cap = max(self.floor, 1 << (int(nbytes) - 1).bit_length())
            s["host"] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            s["dev"] = torch.empty(cap, dtype=torch.uint8, device=self.device)
            s["np"] = s["host"].numpy()
        return s


def device_lib(who, host_path, device=None):
    """The preamble of a class that runs on the GPU -> (libcrnn_mi355x, the resolved torch device); RuntimeError without a GPU."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("%s needs an AMD GPU (gfx950); the host path is %s" % (who, host_path))
    return native.lib(), torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
