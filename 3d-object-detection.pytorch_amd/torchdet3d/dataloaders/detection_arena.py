"""The detection loader with everything resident on the device: `build_detection_loader` with `data.cache = 'device'`.

`GpuDetectionLoader` over `ObjectronFrames(decode='device')` is bound by its host: a Python loop over the samples runs
MinIoURandomCrop's search (`DetectionAugmentPipeline.boxes`), DataLoader workers read and collate every file again each epoch,
and every batch uploads its bytes and index rows.  A cache of pixels cannot exist here -- a frame is 8 MB and every epoch crops
another part of it -- but a COMPRESSED frame is 0.8 MB and its index 87 KB, and the device decodes a batch from HBM.  So:

`DetectionArena` is filled ONCE from an `ObjectronFrames` that has its `JpegIndex`: every file's bytes in one device uint8 tensor
(read by at most 16 host threads of this process through rotating pinned staging), the index's `infos` and `segs` as device
tensors, every image's filtered boxes and labels flattened into device tensors with a start table.  A file the index keeps on
the host (`reason != 0`) is decoded once, by `dataset._decode_host`, and lies in the same tensor as its RGB frame.  Host numpy
keeps what planning a batch needs: offsets, sizes, `seg_start`, each frame's h, w, block and segment counts.

`ArenaDetectionLoader` walks the sampler's indices in the main process -- no DataLoader, no worker, no file read.  Per batch
the host builds, in vectorised numpy, the `t3d_jpeg_item` table (`plan_arena_batch`: `file_offset` and `seg_offset` point into
the resident tables) and the frame table, uploads both in ONE pinned copy, and enqueues a fixed number of launches:
`index_select` of the batch's `t3d_jpeg_info` rows, `t3d_jpeg_decode_u8` with data = the arena and segs = the resident table,
device-to-device copies of host-decoded frames (only files the index refused; none in a set of baseline files),
`t3d_detect_draw` (csrc/detect_draw.hip: the draws, the crop search, the boxes and the records, bit for bit those of
`DetectionAugmentPipeline.draw` / `.boxes` / `.records` from the same key) and `t3d_detect_augment_u8`.  The test pipeline takes
the same route without the draw: records with no flag, `t3d_augment_crops_u8`, boxes scaled and clipped in vectorised numpy,
`ori_shapes` yielded.  With `crop_decode` (`data.decode_crop`, off by default) the train pipeline's order is upload,
`t3d_detect_draw`, `t3d_detect_roi_plan` (csrc/detect_roi.hip: the drawn records -> the rectangle, item and rewritten record of
every device-decoded frame, one launch, nothing read back), `t3d_jpeg_decode_roi_u8` with the host's whole-frame totals as its
bounds, the copies, `t3d_detect_augment_u8`: only what a crop reads is decoded, and the batches are the same bit for bit.

Yields what `GpuDetectionLoader` yields, bit for bit, with ONE difference: G, the second dimension of `gt_boxes` and
`gt_labels`, is the ARENA's capacity -- the largest box count of any image of the set, at least 1 -- not the batch's largest
count.  Rows past a count are zero and every consumer reads `gt_counts`.  The pinned staging of the fill and of the batches,
the packed upload, `prefetch`, the copy stream and the hand-over to the consumer are staging.py's; `sampler`, `__len__`,
`last_status`, `dataset` and `batch_size` mean what they mean on `GpuDetectionLoader`."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .detection import DET_SAMPLE_DTYPE, _CROP_TAG, resize_boxes
from .jpeg import ITEM_DTYPE, frame_blocks, item_table, launch_decode, launch_decode_roi, starts
from .objectron import resize_records
from .staging import PinnedRing, StagedLoader, device_parts, upload

__all__ = ['DetectionArena', 'ArenaDetectionLoader', 'plan_arena_batch', 'pipeline_cfg', 'key_words', 'detect_draw_host',
           'detect_roi_plan_host', 'DRAW_CFG_LEN', 'MAX_BOXES']

DRAW_CFG_LEN = 34           # include/t3d.h: cfg of t3d_detect_draw, by position
MAX_BOXES = 64              # t3d_ssd_multibox_loss and t3d_detect_draw take no more boxes an image
_MAX_MODES = 16
assert _CROP_TAG == 0x5D3C0A7E11F2          # csrc/detect_draw.h: TAG_LO, TAG_HI


def pipeline_cfg(pipeline):
    """A compiled `DetectionAugmentPipeline` -> the float64 [34] `cfg` of t3d_detect_draw (include/t3d.h lists the positions)."""
    c = np.zeros(DRAW_CFG_LEN, np.float64)
    ph = pipeline.photo or dict(delta=0., contrast=(1., 1.), saturation=(1., 1.), hue=0.)
    c[0] = pipeline.photo is not None
    c[1], c[2:4], c[4:6], c[6] = ph['delta'], ph['contrast'], ph['saturation'], ph['hue']
    c[7] = pipeline.p_rot or 0.0
    ex = pipeline.expand or dict(ratio=(1., 1.), p=0.)
    c[8:10], c[10] = ex['ratio'], ex['p']
    if pipeline.crop is not None:
        modes = pipeline.crop['modes']
        if len(modes) > _MAX_MODES:
            raise NotImplementedError(f'MinIoURandomCrop: {len(modes)} modes (t3d_detect_draw takes {_MAX_MODES})')
        c[11], c[12], c[14] = 1, pipeline.crop['min_size'], len(modes)
        c[15:15 + len(modes)] = modes
    # `iou.min() < mode`: a float32 against a Python float -- float32 where the installed numpy treats the Python float as weak
    c[13] = (np.float32(1) + 0.1).dtype == np.float32
    c[31], c[32], c[33] = pipeline.p_flip, pipeline.size[0], pipeline.size[1]
    return c


def key_words(key):
    """(seed, epoch, rank, batch) -> the uint32 words numpy's SeedSequence makes of those integers: each as its 32-bit words,
    low word first, at least one."""
    out = []
    for v in key:
        v = int(v)
        if v < 0:
            raise ValueError(f'a key holds non-negative integers, not {v}')
        out.append(v & 0xFFFFFFFF)
        v >>= 32
        while v:
            out.append(v & 0xFFFFFFFF)
            v >>= 32
    if len(out) > 16:
        raise ValueError(f'the key makes {len(out)} words; t3d_detect_draw takes 16')
    return np.asarray(out, np.uint32)


def detect_draw_host(pipeline, key, frames, boxes, labels, box_start, G):
    """`t3d_detect_draw_host`: the draws, boxes and records of one batch on the CPU (no GPU is touched).  frames int64 [B, 4] =
    (offset, h, w, dataset index); boxes float32 [n, 4], labels int32 [n], box_start int64 [images + 1].
    -> (records [B] DET_SAMPLE_DTYPE, gt_boxes float32 [B, G, 4], gt_labels int32 [B, G], gt_counts int32 [B], diag int32 [B, 2])."""
    from .. import _native as N
    cfg, words = pipeline_cfg(pipeline), key_words(key)
    frames = np.ascontiguousarray(frames, np.int64).reshape(-1, 4)
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    labels, box_start = np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(box_start, np.int64)
    B = len(frames)
    rec = np.full(B, 0, DET_SAMPLE_DTYPE)
    gb, gl = np.full((B, G, 4), np.nan, np.float32), np.full((B, G), -1, np.int32)
    gc, diag = np.full(B, -1, np.int32), np.full((B, 2), -7, np.int32)
    rc = N.lib().t3d_detect_draw_host(cfg.ctypes.data, len(cfg), words.ctypes.data, len(words), frames.ctypes.data, B, boxes.ctypes.data,
                                      labels.ctypes.data, box_start.ctypes.data, len(box_start) - 1, len(labels), int(G), rec.ctypes.data,
                                      gb.ctypes.data, gl.ctypes.data, gc.ctypes.data, diag.ctypes.data, None)
    if rc != 0:
        raise RuntimeError(f't3d_detect_draw_host failed with code {rc}')
    return rec, gb, gl, gc, diag


def detect_roi_plan_host(records, infos, items, src_bytes, sample=None):
    """`t3d_detect_roi_plan_host`: from drawn records to the rectangle decode's tables on the CPU (no GPU is touched).  records
    [B] DET_SAMPLE_DTYPE; infos [n] INFO_DTYPE and items [n] ITEM_DTYPE, the frames' index rows and whole-frame items; sample
    int32 [n]: the record of each item (None: item j, record j).
    -> (records rewritten (a copy), roi items [n] ITEM_DTYPE, rects int32 [n, 12], diag int32 [n, 2] = (pixels, blocks))."""
    from .. import _native as N
    rec = np.array(records, DET_SAMPLE_DTYPE).reshape(-1)
    infos, items = np.ascontiguousarray(infos).reshape(-1), np.ascontiguousarray(items, ITEM_DTYPE).reshape(-1)
    n = len(items)
    if infos.dtype.itemsize != 864 or len(infos) != n:
        raise ValueError('infos: one t3d_jpeg_info row an item')
    sample = None if sample is None else np.ascontiguousarray(sample, np.int32).reshape(n)
    out, rects, diag = np.zeros(n, ITEM_DTYPE), np.full((n, 12), -1, np.int32), np.full((n, 2), -7, np.int32)
    rc = N.lib().t3d_detect_roi_plan_host(rec.ctypes.data, len(rec), None if sample is None else sample.ctypes.data, infos.ctypes.data,
                                          items.ctypes.data, n, int(src_bytes), out.ctypes.data, rects.ctypes.data, diag.ctypes.data, None)
    if rc != 0:
        raise RuntimeError(f't3d_detect_roi_plan_host failed with code {rc}')
    return rec, out, rects, diag


def plan_arena_batch(idx, file_off, size, seg_start, h, w, blocks, nseg):
    """Pure numpy: the tables of one t3d_jpeg_decode_u8 call over RESIDENT files.  idx: the batch's dataset indices (files the
    device decodes); the other arguments are the arena's per-file host arrays.  -> dict(items [len(idx)] ITEM_DTYPE, frames int64
    [len(idx), 4] = (out offset, h, w, dataset index), out_bytes, total_blocks, max_segs, max_blocks).  `out_offset` and
    `block_offset` are prefix sums of the known frame sizes -- what `plan_batch` computes from the rows themselves --
    `file_offset` and `seg_offset` point into the resident tables."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    hh, ww = h[idx].astype(np.int64), w[idx].astype(np.int64)
    nb = hh * ww * 3
    bl = blocks[idx].astype(np.int64)
    items = item_table(file_off[idx], size[idx], starts(nb), seg_start[idx], bl)
    frames = np.stack([items['out_offset'], hh, ww, idx], 1) if len(idx) else np.zeros((0, 4), np.int64)
    return dict(items=items, frames=frames, out_bytes=int(nb.sum()), total_blocks=int(bl.sum()),
                max_segs=int(nseg[idx].max()) if len(idx) else 1, max_blocks=int(bl.max()) if len(idx) else 1)


class DetectionArena:
    """A whole `ObjectronFrames` resident on the device (the module's docstring).  `plan()` is host only: it reads nothing but
    the index and the annotations, decodes the files the index keeps on the host, and raises ValueError when the set does not
    fit `max_gb` (GiB, the meaning and default of the regression cache's `data.cache_max_gb`) or an image has more than 64
    boxes -- before anything is allocated.  `fill()` then reads the files and uploads everything."""
    STAGING = 64 << 20          # bytes of one pinned staging buffer (a larger file gets a buffer of its own size)

    def __init__(self, frames, max_gb=32, threads=16):
        if getattr(frames, 'index', None) is None:
            raise RuntimeError('DetectionArena needs the JPEG index of its ObjectronFrames: call build_index() first')
        self.frames, self.max_gb, self.threads = frames, max_gb, max(1, min(int(threads), 16))
        self.data = None
        self.plan()

    def plan(self):
        fr, index = self.frames, self.frames.index
        n = len(fr)
        index.check(fr.root)                                     # a changed size or mtime raises, naming the file
        self.kind = (np.asarray(index.reason) != 0).astype(np.int64)          # 1: the arena holds the host-decoded RGB frame
        infos = index.infos
        self.h, self.w = np.array(infos['h'], np.int64), np.array(infos['w'], np.int64)
        self.size = np.array(index.size, np.int64)
        self._host_frames = {}
        for i in np.flatnonzero(self.kind):
            f = np.ascontiguousarray(fr._decode_host(fr.root + '/' + fr.files[i]), np.uint8)
            self._host_frames[int(i)] = f
            self.h[i], self.w[i], self.size[i] = f.shape[0], f.shape[1], f.size
        self.file_off = np.cumsum(self.size) - self.size
        self.seg_start = np.array(index.seg_start[:-1], np.int64)
        dev = self.kind == 0
        self.nseg = np.where(dev, infos['nseg'], 0).astype(np.int64)
        self.blocks = np.where(dev, frame_blocks(infos), 0)
        # a whole frame's share of t3d_jpeg_decode_roi_u8's grid bounds: upper bounds of any rectangle's
        per_row = (np.maximum(infos['mcus_x'].astype(np.int64), 1) - 1) // np.maximum(infos['seg_mcus'], 1) + 2
        self.lanes = np.where(dev, infos['mcus_y'] * per_row, 0).astype(np.int64)
        self.runs = np.where(dev, self.h * ((self.w + 3) // 4), 0).astype(np.int64)
        counts = np.array([len(l) for l in fr._labels], np.int64).reshape(-1)
        self.box_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.boxes = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in fr._boxes] + [np.zeros((0, 4), np.float32)])
        self.labels = np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in fr._labels] + [np.zeros(0, np.int32)])
        self.G = int(max(counts.max() if n else 0, 1))
        if self.G > MAX_BOXES:
            i = int(counts.argmax())
            raise ValueError(f'{fr.files[i]} has {self.G} boxes; t3d_ssd_multibox_loss takes {MAX_BOXES} an image')
        self.bytes = (int(self.size.sum()) + infos.size * infos.dtype.itemsize + len(index.segs) * index.segs.dtype.itemsize
                      + self.boxes.nbytes + self.labels.nbytes + self.box_start.nbytes)
        budget = int(float(self.max_gb) * 2 ** 30)
        if self.bytes > budget:
            raise ValueError(f'data.cache: {n} files and their index need {self.bytes} bytes ({self.bytes / 2 ** 30:.3f} GiB), over the '
                             f'budget data.cache_max_gb = {self.max_gb} ({budget} bytes); there is no partial cache')

    def __len__(self):
        return len(self.frames)

    def fill(self, device=None):
        """Read every file (at most 16 threads of this process, rotating pinned staging) and upload the tables.  -> self."""
        if not torch.cuda.is_available():
            raise RuntimeError("data.cache = 'device' keeps the files on the GPU (no CPU fallback)")
        fr, index = self.frames, self.frames.index
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        total = int(self.size.sum())
        self.data = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        # chunks of consecutive files that fit one staging buffer
        chunks, start, acc = [], 0, 0
        for i, s in enumerate(self.size):
            if acc and acc + s > self.STAGING:
                chunks.append((start, i))
                start, acc = i, 0
            acc += int(s)
        if len(self.size):
            chunks.append((start, len(self.size)))
        ring = PinnedRing(1)

        def read(i, view, base):
            at, n = int(self.file_off[i] - base), int(self.size[i])
            if self.kind[i]:
                view[at:at + n] = self._host_frames[i].reshape(-1)
                return
            path = os.path.join(str(fr.root), fr.files[i])
            with open(path, 'rb') as f:
                got = f.readinto(memoryview(view[at:at + n]))
                more = f.read(1)
            if got != n or more:
                raise RuntimeError(f'{path} changed since it was indexed ({n} bytes in the index): rebuild the index')
        with ThreadPoolExecutor(max_workers=self.threads) as ex:
            for a, b in chunks:
                base, nbytes = int(self.file_off[a]), int(self.size[a:b].sum())
                slot = ring.take(nbytes)
                view = slot.host.numpy()
                list(ex.map(lambda i: read(i, view, base), range(a, b)))
                self.data[base:base + nbytes].copy_(slot.host[:nbytes], non_blocking=True)
                slot.uploaded(torch.cuda.current_stream(dev))
        self._host_frames = {}

        def up(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).to(dev)
        self.infos = up(np.asarray(index.infos)).view(-1, index.infos.dtype.itemsize) if len(fr) else up(np.zeros(0, np.uint8))
        self.segs = up(np.asarray(index.segs))
        self.d_boxes, self.d_labels, self.d_box_start = up(self.boxes), up(self.labels), up(self.box_start)
        torch.cuda.synchronize(dev)                # every later stream finds the tables complete
        return self


class ArenaDetectionLoader(StagedLoader):
    """Batches for the detector from a filled `DetectionArena` (the module's docstring): the tuples of `GpuDetectionLoader`, with
    G = `arena.G`.  indices: the dataset indices this loader walks, in order, when there is no sampler (None: all of them);
    `dataset` is what `GpuDetectionLoader.dataset` would be (the frames, or the Subset of them).
    crop_decode (`data.decode_crop`): with a random pipeline the draw runs BEFORE the decode, `t3d_detect_roi_plan` turns its
    records into rectangles on the device, and `t3d_jpeg_decode_roi_u8` decodes of every frame only what its crop reads; the
    batches are the same bit for bit.  `last_crop_diag` then holds the batch's device int32 [n, 2]: pixels and 8x8 blocks asked
    for, a row per device-decoded frame.  The test pipeline reads whole frames and ignores the flag."""

    def __init__(self, arena, pipeline, batch_size, sampler=None, indices=None, drop_last=False, seed=0, rank=0, prefetch=1,
                 dataset=None, crop_decode=False):
        if arena.data is None:
            raise RuntimeError('ArenaDetectionLoader needs a filled arena: call DetectionArena.fill() first')
        super().__init__(prefetch, min_staging=1 << 14)
        self.arena, self.pipeline, self.batch_size = arena, pipeline, int(batch_size)
        self.seed, self.rank, self.drop_last = int(seed), int(rank), bool(drop_last)
        self.sampler = sampler
        self.indices = np.arange(len(arena), dtype=np.int64) if indices is None else np.asarray(list(indices), np.int64)
        self.dataset = arena.frames if dataset is None else dataset
        self.decode, self.last_status = 'arena', None
        self.crop_decode, self.last_crop_diag = bool(crop_decode), None
        self._cfg = pipeline_cfg(pipeline)

    def _order(self):
        return np.fromiter(iter(self.sampler), np.int64) if self.sampler is not None else self.indices

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.indices)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def host_plan(self, idx):
        """The host half of one batch, vectorised numpy only.  idx: the batch's dataset indices.  -> (parts: the uint8 arrays of
        the one upload -- frames | items | gather indices [| records | boxes | labels | counts | shapes for the test pipeline]
        [| batch positions of the device-decoded files with crop_decode] --
        plan of the device-decoded files, positions of the host-decoded frames)."""
        A = self.arena
        idx = np.asarray(idx, np.int64)
        B = len(idx)
        hh, ww = A.h[idx], A.w[idx]
        nb = hh * ww * 3
        out_off = starts(nb)
        frames = np.stack([out_off, hh, ww, idx], 1)
        on_dev = np.flatnonzero(A.kind[idx] == 0)
        plan = plan_arena_batch(idx[on_dev], A.file_off, A.size, A.seg_start, A.h, A.w, A.blocks, A.nseg)
        plan['items']['out_offset'] = out_off[on_dev]
        plan['out_bytes'], plan['total_segs'] = int(nb.sum()), A.segs.numel() // 16
        dev_idx = idx[on_dev]
        plan['max_lanes'] = int(A.lanes[dev_idx].max()) if len(dev_idx) else 1
        plan['max_runs'] = int(A.runs[dev_idx].max()) if len(dev_idx) else 1
        parts = [frames.reshape(-1).view(np.uint8), plan['items'].view(np.uint8), dev_idx.view(np.uint8)]
        if not self.pipeline.random:
            G = A.G
            rec = resize_records(frames)
            start, cnt = A.box_start[idx], A.box_start[idx + 1] - A.box_start[idx]
            row = np.repeat(np.arange(B), cnt)
            col = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            src = np.repeat(start, cnt) + col
            gb, gl = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32)
            gb[row, col] = resize_boxes(A.boxes[src], row, hh, ww, self.pipeline.size)
            gl[row, col] = A.labels[src]
            parts += [rec.view(np.uint8), gb.reshape(-1).view(np.uint8), gl.reshape(-1).view(np.uint8), cnt.astype(np.int32).view(np.uint8),
                      np.stack([hh, ww], 1).astype(np.int32).reshape(-1).view(np.uint8)]
        elif self.crop_decode:
            parts.append(on_dev.astype(np.int32).view(np.uint8))
        return parts, plan, np.flatnonzero(A.kind[idx] != 0), frames

    def finish(self, idx, key_tail, prefetch=None):
        """The batch of dataset indices `idx` -> the device tuple, enqueued on the copy stream (prefetch >= 1: the ready event is
        appended) or on the current stream (prefetch 0)."""
        return self._public(*self._finish(idx, key_tail, prefetch))

    def _finish(self, idx, key_tail, prefetch=None):
        """-> (the device tuple, ready event or None)."""
        from .. import _native as N
        prefetch = self.prefetch if prefetch is None else prefetch
        A = self.arena
        parts, plan, on_host, frames = self.host_plan(idx)
        B, G = len(idx), A.G
        oh, ow = self.pipeline.size
        dev = A.data.device
        stream = self._stream(dev, prefetch)
        part = upload(self._ring, parts, stream, dev).part
        with torch.cuda.stream(stream):
            imgs = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=dev)
            src = torch.empty(max(plan['out_bytes'], 1), dtype=torch.uint8, device=dev)
            n_dev = len(plan['items'])
            crop = self.crop_decode and self.pipeline.random
            infos = A.infos.index_select(0, part(2, torch.int64, n_dev)) if n_dev else None
            if crop:                               # the draw reads no pixel: it runs first and says what to decode
                rec, gb, gl, gc = self._draw(part, B, key_tail, dev)
                if n_dev:
                    items, rects, diag = device_parts([n_dev * ITEM_DTYPE.itemsize, n_dev * 48, n_dev * 8], dev)
                    N.call('t3d_detect_roi_plan', N.ptr(rec), B, N.ptr(part(3, torch.uint8, -1)), N.ptr(infos), N.ptr(part(1, torch.uint8, -1)),
                           n_dev, src.numel(), N.ptr(items), N.ptr(rects), N.ptr(diag), N.stream())
                    self.last_status = launch_decode_roi(A.data, infos, A.segs, items, rects, plan, src)
                    self.last_crop_diag = diag.view(torch.int32).view(n_dev, 2)
            elif n_dev:
                self.last_status = launch_decode(A.data, infos, A.segs, part(1, torch.uint8, -1), plan, src)
            if not n_dev:
                self.last_status = torch.zeros(0, dtype=torch.int32, device=dev)
            for k in on_host:                      # frames the host had to decode (files the index refused) lie in the arena as they are
                at, to, n = int(A.file_off[idx[k]]), int(frames[k, 0]), int(A.size[idx[k]])
                src[to:to + n].copy_(A.data[at:at + n], non_blocking=True)
            if self.pipeline.random:
                if not crop:
                    rec, gb, gl, gc = self._draw(part, B, key_tail, dev)
                N.call('t3d_detect_augment_u8', N.ptr(src), src.numel(), N.ptr(rec), N.ptr(imgs), B, oh, ow, N.stream())
                out = (imgs, gb.view(torch.float32).view(B, G, 4), gl.view(torch.int32).view(B, G), gc.view(torch.int32))
            else:
                N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(part(3, torch.uint8, -1)), N.ptr(imgs), B, oh, ow, N.stream())
                out = (imgs, part(4, torch.float32, B, G, 4), part(5, torch.int32, B, G), part(6, torch.int32, B), part(7, torch.int32, B, 2))
        return out, self._ready(stream, prefetch)

    def _draw(self, part, B, key_tail, dev):
        """Enqueue t3d_detect_draw for the uploaded frame table -> uint8 device views (records, gt_boxes, gt_labels, gt_counts)."""
        from .. import _native as N
        A, G = self.arena, self.arena.G
        epoch = int(getattr(self.sampler, 'epoch', 0))
        words = key_words((self.seed, epoch, self.rank) + tuple(key_tail))
        rec, gb, gl, gc, diag = device_parts([B * 80, B * G * 16, B * G * 4, B * 4, B * 8], dev)
        N.call('t3d_detect_draw', self._cfg.ctypes.data, len(self._cfg), words.ctypes.data, len(words), N.ptr(part(0, torch.uint8, -1)),
               B, N.ptr(A.d_boxes), N.ptr(A.d_labels), N.ptr(A.d_box_start), len(A), len(A.labels), G, N.ptr(rec), N.ptr(gb),
               N.ptr(gl), N.ptr(gc), N.ptr(diag), N.stream())
        return rec, gb, gl, gc

    def __iter__(self):
        order, bs = self._order(), self.batch_size
        yield from self._batches((order[b * bs:(b + 1) * bs] for b in range(len(self))), self._finish)
