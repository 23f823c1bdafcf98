"""Device-side input path: page images go to the GPU once as uint8 together with a small table of word boxes, and one launch of
crnn_ingest_crops (csrc/ingest.hip) builds the normalised (B, imgh, imgw, 1) fp32 batch the forward reads -- bit-identical to what
`data.open_img` + `data.norm` produce on the host (reference utils.py:364-416).  The host keeps the image file decoding, the slicing rules
of `page[y0:y1, x0:x1]` and every random decision of the padding (`plan_crop` draws from np.random exactly as `open_img` does), so the
kernel knows nothing about random numbers and serves augmented batches as well (the augmentation itself is a second launch on the uint8
batch: crnn_mi355x/augment.py).

    ing = DeviceIngest((100, 32, 1))
    x, words = ing.pages([page], [[(None, x0, y0, x1, y1), ...]])      # x: device tensor (n, 100, 32, 1)
    gen = DeviceReadf(img_size=(100, 32, 1), normed=True, batch_size=64, classes=classes, transform_p=0.).run_generator(names, bboxs=b)
"""
import ctypes

import numpy as np

from . import native
from .data import Readf, norm, read_img, _word_of
from .pages import StagingSlots, arena_layout, device_lib, pack_arena, upload_pages


class crnn_crop_item(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_crop_item."""
    _fields_ = ([("page_off", ctypes.c_long)]
                + [(n, ctypes.c_int) for n in ("rows", "cols", "stride", "r0", "r1", "c0", "c1", "b0", "b1", "p0", "p1", "upscale")]
                + [(n, ctypes.c_double) for n in ("up_scale0", "up_scale1", "out_scale0", "out_scale1")])


ITEM_DTYPE = np.dtype([(n, {ctypes.c_long: np.dtype("l"), ctypes.c_int: np.intc, ctypes.c_double: np.float64}[t])
                       for n, t in crnn_crop_item._fields_], align=True)
assert ITEM_DTYPE.itemsize == ctypes.sizeof(crnn_crop_item)


def _place(size, target, axis, p, strict):
    """data._pad_axis as (offset of the content, padded size); same draws from np.random, in the same order."""
    delta = target - size
    if delta <= 2:
        return 0, size
    r = round(np.random.uniform(0, 1), 1)
    randomise = (r < p) if strict else (r <= p)
    if randomise and p > 0.:
        c = int(np.random.choice(list(range(2, delta))))
        return c - 1, target - 1
    if axis == 1:
        return 0, target
    return delta // 2, size + 2 * (delta // 2)


def plan_crop(hc, wc, img_size, p=0.):
    """Shape-only part of data.open_img for a crop of hc rows x wc columns: -> (upscale, (s0, s1), (b0, b1, p0, p1)): whether the rotated
    crop (wc, hc) is first scaled by 1.5, the content's size, its offset in the padded image and that image's size (axis 0 = time).
    Draws from np.random in exactly the order and count open_img does; p = 0 gives the flush (axis 1) / centred (axis 0) placement."""
    T0, T1 = int(img_size[0]), int(img_size[1])
    s0, s1 = int(wc), int(hc)
    up = s0 <= T0 // 2 and s1 <= T1 // 2
    if up:
        s0, s1 = int(s0 * 1.5), int(s1 * 1.5)
    b1, p1 = _place(s1, T1, 1, p, True)
    b0, p0 = _place(s0, T0, 0, p, False)
    return up, (s0, s1), (b0, b1, p0, p1)


def plan_crops(hc, wc, img_size):
    """plan_crop(p=0) over arrays of crop shapes -> (upscale, s0, s1, b0, b1, p0, p1) arrays; np.random advances as the per-crop calls would
    (one uniform per padded axis: open_img draws it even when p = 0 ignores it)."""
    T0, T1 = int(img_size[0]), int(img_size[1])
    s0, s1 = np.asarray(wc, dtype=np.int64), np.asarray(hc, dtype=np.int64)
    up = (s0 <= T0 // 2) & (s1 <= T1 // 2)
    s0, s1 = np.where(up, (3 * s0) >> 1, s0), np.where(up, (3 * s1) >> 1, s1)
    d0, d1 = T0 - s0, T1 - s1
    draws = int((d0 > 2).sum() + (d1 > 2).sum())
    if draws:
        np.random.uniform(0, 1, size=draws)
    p1 = np.where(d1 > 2, T1, s1)
    b0 = np.where(d0 > 2, d0 // 2, 0)
    p0 = s0 + 2 * b0
    return up, s0, s1, b0, np.zeros_like(b0), p0, p1


def plan_rects(rects, img_size, transform_p=0.):
    """rects (n, 4) = r0, r1, c0, c1 -> plan_crops' tuple of arrays; transform_p > 0 draws crop by crop, as the serial open_img loop does."""
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    hc, wc = rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2]
    if not transform_p > 0.:
        return plan_crops(hc, wc, img_size)
    rows = [(up, s[0], s[1]) + o for up, s, o in (plan_crop(int(h), int(w), img_size, p=transform_p) for h, w in zip(hc, wc))]
    return tuple(np.array(col) for col in zip(*rows)) if rows else tuple(np.zeros(0, np.int64) for _ in range(7))


def box_slices(box, shape):
    """(word|None, x0, y0, x1, y1) -> (r0, r1, c0, c1) of page[box[1]:box[3], box[2]:box[4]] (negative and out-of-range bounds as Python
    slicing resolves them); ValueError when the slice is empty."""
    def bound(v):
        return None if v is None else int(v)
    r0, r1, _ = slice(bound(box[1]), bound(box[3])).indices(int(shape[0]))
    c0, c1, _ = slice(bound(box[2]), bound(box[4])).indices(int(shape[1]))
    if r1 <= r0 or c1 <= c0:
        raise ValueError("empty crop: box %r on a %d x %d page" % (tuple(box[1:5]), shape[0], shape[1]))
    return r0, r1, c0, c1


def build_table(pages, offsets, page_index, rects, plans, img_size, out=None):
    """The crnn_crop_item table of n crops: page_index (n,), rects (n, 4) = r0, r1, c0, c1, plans = (upscale, s0, s1, b0, b1, p0, p1) arrays
    as plan_crops returns them.  The scale factors are n_in / float(n_out) in Python arithmetic, as data._linear_taps computes them."""
    T0, T1 = int(img_size[0]), int(img_size[1])
    n = len(page_index)
    t = np.zeros(n, ITEM_DTYPE) if out is None else out[:n]
    if n == 0:
        return t
    pi = np.asarray(page_index, dtype=np.int64)
    rects = np.asarray(rects, dtype=np.int64).reshape(n, 4)
    up, s0, s1, b0, b1, p0, p1 = [np.asarray(a) for a in plans]
    shapes = np.array([pg.shape for pg in pages], dtype=np.int64).reshape(-1, 2)
    t["page_off"] = np.asarray(offsets, dtype=np.int64)[pi]
    t["rows"], t["cols"], t["stride"] = shapes[pi, 0], shapes[pi, 1], shapes[pi, 1]
    t["r0"], t["r1"], t["c0"], t["c1"] = rects[:, 0], rects[:, 1], rects[:, 2], rects[:, 3]
    t["b0"], t["b1"], t["p0"], t["p1"], t["upscale"] = b0, b1, p0, p1, up
    wc, hc = (rects[:, 3] - rects[:, 2]).astype(np.float64), (rects[:, 1] - rects[:, 0]).astype(np.float64)
    t["up_scale0"] = np.where(up, wc / s0.astype(np.float64), 1.0)       # float64 division = Python's n_in / float(n_out)
    t["up_scale1"] = np.where(up, hc / s1.astype(np.float64), 1.0)
    t["out_scale0"] = p0.astype(np.float64) / float(T0)
    t["out_scale1"] = p1.astype(np.float64) / float(T1)
    return t


def norm_table(normed=True, mean=118.24236953981779, std=36.72835353999682):
    """grey value -> network input, 256 fp32: data.norm evaluated on every uint8 value, or the identity."""
    grey = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(norm(grey, mean, std) if normed else grey, dtype=np.float32)


class DeviceIngest:
    """Word crops -> device batch.  Per call: the pages and the box table are written into one page-locked buffer, copied to the device in one
    asynchronous transfer, and one kernel launch builds the batch on the current stream.  Two staging slots: a slot's host buffer is rewritten
    only after its previous copy has finished (the Engine.stage pattern); copy and kernel are ordered by the stream, so successive calls belong
    on one stream."""
    _SLOTS = 2

    def __init__(self, img_size, normed=True, mean=118.24236953981779, std=36.72835353999682, device=None):
        import torch
        self.lib, self.device = device_lib("DeviceIngest", "data.Readf", device)
        self.img_size = tuple(img_size)
        self.T0, self.T1 = int(img_size[0]), int(img_size[1])
        self.table = torch.from_numpy(norm_table(normed, mean, std)).to(self.device)
        self._slot = StagingSlots(self.device, self._SLOTS).take

    def upload(self, pages):
        """Pages -> PageArena (pages.py: the arena every page stage shares) on this ingest's device, for crops(..., arena=) and
        WordDetector.detect(arena=): the pages go up once, and each crop launch afterwards uploads its box table only."""
        return upload_pages(pages, self.device)

    def crops(self, pages, page_index, rects, plans, batch=None, return_u8=False, arena=None):
        """pages: list of (H, W) uint8 arrays; crop k is pages[page_index[k]][r0:r1, c0:c1] with rects[k] = (r0, r1, c0, c1), placed as plans
        (plan_crops' tuple of arrays) says.  -> device fp32 (batch or n, imgh, imgw, 1), rows past n zero [, the uint8 pixels before the table].
        arena: a PageArena from `upload` -- its pages are used (`pages` may be None) and only the table is copied."""
        import torch
        from .engine import _ptr, _stream
        n = len(page_index)
        B = n if batch is None else int(batch)
        if B < 1 or n > B:
            raise ValueError("%d crops do not fit a batch of %d" % (n, B))
        if arena is not None:
            nbytes = n * ITEM_DTYPE.itemsize
            with torch.cuda.device(self.device):
                s = self._slot(max(nbytes, 1))
                build_table(arena.pages, arena.offsets, page_index, rects, plans, self.img_size, out=s["np"][:nbytes].view(ITEM_DTYPE))
                if nbytes:
                    s["dev"][:nbytes].copy_(s["host"][:nbytes], non_blocking=True)
                    s["copied"].record(torch.cuda.current_stream())
                out = torch.empty((B, self.T0, self.T1, 1), dtype=torch.float32, device=self.device)
                u8 = torch.empty((B, self.T0, self.T1), dtype=torch.uint8, device=self.device) if return_u8 else None
                native.check(self.lib.crnn_ingest_crops(ctypes.c_void_p(arena.dev.data_ptr()), arena.nbytes, ctypes.c_void_p(s["host"].data_ptr()),
                                                        ctypes.c_void_p(s["dev"].data_ptr()), n, B, self.T0, self.T1, _ptr(self.table), _ptr(out),
                                                        _ptr(u8), _stream()), "ingest_crops")
            return (out, u8) if return_u8 else out
        pages = [np.ascontiguousarray(pg) for pg in pages]
        offs, arena_bytes = arena_layout(pages)
        total = arena_bytes + n * ITEM_DTYPE.itemsize
        with torch.cuda.device(self.device):
            s = self._slot(max(total, 1))
            pack_arena(pages, out=s["np"])
            tab = s["np"][arena_bytes:total].view(ITEM_DTYPE)
            build_table(pages, offs, page_index, rects, plans, self.img_size, out=tab)
            if total:
                s["dev"][:total].copy_(s["host"][:total], non_blocking=True)
                s["copied"].record(torch.cuda.current_stream())
            out = torch.empty((B, self.T0, self.T1, 1), dtype=torch.float32, device=self.device)
            u8 = torch.empty((B, self.T0, self.T1), dtype=torch.uint8, device=self.device) if return_u8 else None
            native.check(self.lib.crnn_ingest_crops(ctypes.c_void_p(s["dev"].data_ptr()), arena_bytes, ctypes.c_void_p(s["host"].data_ptr() + arena_bytes),
                                                    ctypes.c_void_p(s["dev"].data_ptr() + arena_bytes), n, B, self.T0, self.T1, _ptr(self.table), _ptr(out),
                                                    _ptr(u8), _stream()), "ingest_crops")
        return (out, u8) if return_u8 else out

    def plan(self, rects, transform_p=0.):
        """plan_rects for this image size."""
        return plan_rects(rects, self.img_size, transform_p)

    def pages(self, pages, boxes, transform_p=0., batch=None, return_u8=False):
        """pages: list of (H, W) uint8 arrays; boxes: per page a list of (word|None, x0, y0, x1, y1), sliced as page[b[1]:b[3], b[2]:b[4]].
        -> (device fp32 (batch or n, imgh, imgw, 1), words) [with return_u8: ((fp32, uint8), words)]."""
        index, rects, words = [], [], []
        for k, (pg, bl) in enumerate(zip(pages, boxes)):
            for b in bl:
                index.append(k)
                rects.append(box_slices(b, pg.shape))
                words.append(b[0] if b[0] is not None else "-")
        return self.crops(pages, index, rects, self.plan(rects, transform_p), batch=batch, return_u8=return_u8), words

    def _jpeg(self):
        if getattr(self, "_decoder", None) is None:
            from .jpeg import JpegDecoder
            self._decoder = JpegDecoder(self.device)
        return self._decoder

    def decoded(self, files, names=None):
        """Image files (byte strings or names) -> PageArena of their grey pages, decoded on the device (jpeg.JpegDecoder: baseline JPEG there,
        everything else by read_img on the host, in the same upload).  Reads the per-file status back -- one small synchronising copy per call,
        4 bytes per file -- and raises ValueError naming the first file whose data is corrupt or truncated."""
        from .jpeg import CORRUPT, TRUNCATED
        arena, status, _ = self._jpeg().decode(files)
        bad = np.flatnonzero(status.cpu().numpy() & (CORRUPT | TRUNCATED))
        if len(bad):
            which = (names if names is not None else files)[int(bad[0])]
            raise ValueError("corrupt or truncated JPEG data: %s" % (which if isinstance(which, str) else "file %d" % int(bad[0])))
        return arena

    def files(self, names, transform_p=0., batch=None, return_u8=False, decode="host"):
        """One word per image file (mjsynth, IAM words), every file a whole-image box.  decode="host": decoded with data.read_img on the host.
        decode="device": the files' bytes go up and are decoded there (`decoded`); bit-equal on greyscale files, and on colour files equal
        but for the grey of exact rounding ties (jpeg.py)."""
        if decode not in ("host", "device"):
            raise ValueError("decode is 'host' or 'device', not %r" % (decode,))
        if decode == "device":
            arena = self.decoded(names)
            rects = [(0, pg.shape[0], 0, pg.shape[1]) for pg in arena.pages]
            words = [_word_of(name).lower() for name in names]
            return self.crops(None, list(range(len(rects))), rects, self.plan(rects, transform_p), batch=batch, return_u8=return_u8, arena=arena), words
        pages = [read_img(name) for name in names]
        rects = [(0, pg.shape[0], 0, pg.shape[1]) for pg in pages]
        words = [_word_of(name).lower() for name in names]
        return self.crops(pages, list(range(len(pages))), rects, self.plan(rects, transform_p), batch=batch, return_u8=return_u8), words


def _decode_files(names):
    """Worker entry (module level: picklable under the spawn start method)."""
    return [read_img(name) for name in names]


class FileRef:
    """An image file still encoded (DeviceReadf(device_decode=True)): its name, its bytes and the (rows, cols) its header states, so that crops
    are planned before anything is decoded."""

    def __init__(self, name, data):
        from .jpeg import header_size
        self.name, self.data = name, data
        self.shape = header_size(data)
        if self.shape is None:                                 # no JPEG: the host decodes it later; its size from the container's header
            import io
            from PIL import Image
            w, h = Image.open(io.BytesIO(data)).size
            self.shape = (h, w)


def _read_files(names):
    """Worker entry of device_decode: the files' bytes, nothing decoded."""
    out = []
    for name in names:
        with open(name, "rb") as fh:
            out.append(FileRef(name, fh.read()))
    return out


class DeviceReadf(Readf):
    """Readf whose batches are built on the device: run_generator yields the same dictionaries with 'the_input' as a device fp32 tensor
    (B,) + img_size -- same visiting order, first-pass tail rule, labels, lengths and source_str as the serial Readf (workers=0), and for
    transform_p > 0 the same draws from np.random, so under one seed the images are the serial loop's bit for bit.  Rows past a short tail
    batch's items are zero (Readf leaves them undefined).  `workers=N` decodes the image files in N processes, in order and a bounded
    number ahead (the one piece of work left on the host); everything after the decoding is the same for any worker count.
    `device_decode=True`: the files are read, not decoded -- crops are planned from the header's dimensions, `workers=N` only read bytes, and
    each batch's files are decoded on the device in front of its crop launch (DeviceIngest.decoded: baseline JPEG there, anything else by
    read_img on the host; one 4-byte-per-file status read-back per batch, after which a corrupt or truncated file raises ValueError with its
    name).  Same labels, lengths, source_str, visiting order and np.random draws; the images are bit-equal on greyscale files, and on colour
    files differ at most by the grey of exact rounding ties (jpeg.py).  A page file with many boxes is decoded once per batch that cuts from
    it: the mode is meant for one-word files.
    `augment` (an augment.AugmentPolicy): every emitted batch is augmented on the device, in a second launch on the same stream, with the
    items the policy draws for it -- the batches of Readf(augment=policy) under the same seeds, bit for bit."""

    def __init__(self, *args, device=None, device_decode=False, **kwargs):
        super().__init__(*args, **kwargs)
        self._device, self._ingest, self._augmenter = device, None, None
        self._load = _read_files if device_decode else _decode_files

    def _get_ingest(self):
        if self._ingest is None:
            self._ingest = DeviceIngest(self.img_size, normed=self.normed, mean=self.mean, std=self.std, device=self._device)
        return self._ingest

    def _get_augmenter(self):
        if self._augmenter is None:
            from .augment import Augmenter
            self._augmenter = Augmenter(self.img_size, normed=self.normed, mean=self.mean, std=self.std, device=self._get_ingest().device)
        return self._augmenter

    def _decoded(self, names, bboxs):
        """Endless stream of [(name, decoded image), ...] groups in the visiting order: one page, or a run of up to `chunk` one-word files
        (Readf._tasks' grouping); with workers the groups are decoded by the pool, up to 2 * workers of them ahead."""
        def groups():
            while True:
                run = []
                for name in names:
                    whole = bboxs[name][0] == name
                    if whole:
                        run.append(name)
                    if run and (not whole or len(run) == self.chunk):
                        yield run
                        run = []
                    if not whole:
                        yield [name]
                if run:
                    yield run
        if self.workers <= 0:
            for group in groups():
                yield list(zip(group, self._load(group)))
        from collections import deque
        pool, pending, tasks = self._get_pool(), deque(), groups()
        while True:
            while len(pending) < 2 * self.workers:
                group = next(tasks)
                pending.append((group, pool.apply_async(self._load, (group,))))
            group, res = pending.popleft()
            yield list(zip(group, res.get()))

    def _planned(self, names, bboxs):
        """Endless stream of (page, rect, plan row, word) in Readf._instances' order."""
        for group in self._decoded(names, bboxs):
            crops = []                                                 # (page, rect, word) of the group's crops
            for name, page in group:
                boxes = bboxs[name]
                if boxes[0] == name:
                    crops.append((page, (0, page.shape[0], 0, page.shape[1]), _word_of(name).lower()))
                else:
                    crops.extend((page, box_slices(b, page.shape), (b[0] if b[0] is not None else "-")) for b in boxes)
            if not self.transform_p > 0.:
                plan = np.stack(plan_rects([c[1] for c in crops], self.img_size, 0.), axis=1)     # the group at once: p = 0 uses no draw
                for (page, rect, word), row in zip(crops, plan):
                    yield page, rect, row, word
            else:
                for page, rect, word in crops:                         # drawn when the crop is reached, as open_img does
                    yield page, rect, np.stack(plan_rects([rect], self.img_size, self.transform_p), axis=1)[0], word

    def _device_batch(self, items):
        pages, slot_of, index = [], {}, []
        for page, _, _, _ in items:
            k = slot_of.get(id(page))
            if k is None:
                k = slot_of[id(page)] = len(pages)
                pages.append(page)
            index.append(k)
        plans = tuple(np.stack([it[2] for it in items], axis=1))
        rects = [it[1] for it in items]
        arena = None
        if self._load is _read_files:                                  # device_decode: the batch's files are decoded where the crops are cut
            arena, pages = self._get_ingest().decoded([ref.data for ref in pages], [ref.name for ref in pages]), None
        if self.augment is None:
            return self._get_ingest().crops(pages, index, rects, plans, batch=self.batch_size, arena=arena)
        _, u8 = self._get_ingest().crops(pages, index, rects, plans, batch=self.batch_size, return_u8=True, arena=arena)
        return self._get_augmenter().run(u8, self.augment.draw(len(items), self.img_size))

    def run_generator(self, names, downsample_factor=2, bboxs={}):
        if bboxs:
            total = sum(len(v) for v in bboxs.values())
        else:
            bboxs = {name: [name] for name in names}
            total = len(names)
        full_batches, remainder = divmod(total, self.batch_size)
        steps_in = (self.img_size[0] + 4) // downsample_factor - 2
        emitted = 0
        items, words = [], []
        _, Y, in_len, lab_len = self.get_blank_matrices()
        for item in self._planned(names, bboxs):
            slot, word = len(items), item[3]
            items.append(item)
            words.append(word)
            ids = self.make_target(word)
            Y[slot, :len(ids)] = ids
            lab_len[slot] = len(ids)
            in_len[slot] = steps_in
            slot += 1
            tail = emitted == full_batches and slot == remainder
            if not tail and slot != self.batch_size:
                continue
            batch = ({'the_input': self._device_batch(items), 'the_labels': Y, 'input_length': in_len, 'label_length': lab_len,
                      'source_str': np.array(words)}, {'ctc': np.zeros([self.batch_size])})
            if tail:
                yield batch            # short tail of the first pass: the next batch starts with the same items, as Readf's does
            else:
                emitted += 1
                items, words = [], []
                _, Y, in_len, lab_len = self.get_blank_matrices()
                yield batch
