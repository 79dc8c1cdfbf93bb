"""Batches for the detector, finished on the GPU: what `SSD300.loss`, `MultiBoxLoss.from_heads` and `SSD300.detect` take.

A `StagedLoader` (staging.py), as `GpuAugmentLoader` is.  A DataLoader (workers, pinned memory) yields the host side of a batch --
whole frames packed in one buffer plus a descriptor table, boxes and labels (`collate_frames`).  For each batch the main
process draws the parameters, runs the box arithmetic, builds the kernel records, uploads records | boxes | labels | counts
in ONE pinned copy and launches `t3d_detect_augment_u8` once (csrc/detect_augment.hip).  With `prefetch` >= 1 that work runs
on a copy stream `prefetch` batches ahead of the consumer and each batch is handed over with an event the consumer's stream
waits on; `prefetch = 0` does it synchronously on the consumer's stream.  The pinned staging, the packed upload, the copy
stream and that loop are staging.py's.

Yields device tensors `(imgs uint8 [B, oh, ow, 3], gt_boxes float32 [B, G, 4] in input pixels, gt_labels int32 [B, G],
gt_counts int32 [B])`, G the batch's largest count (at least 1), rows past a count zero.  A pipeline that is `Resize` alone
(the config's test pipeline) runs through `t3d_augment_crops_u8` with no flag set -- the 8-bit cv2 resize mmdet's test
path does -- scales the boxes by (ow / w, oh / h) and additionally yields `ori_shapes int32 [B, 2]` = (h, w) of each frame.

The draws are keyed (seed, epoch, rank, batch) and the epoch is read from `sampler.epoch`: `set_epoch` on a DistributedSampler
(what `build_detection_loader` installs, also for one rank) is what advances them; a loader built with `shuffle=True` and no
such sampler repeats its augmentations every epoch, as `GpuAugmentLoader` does.

There is no device cache of pixels (the COMPRESSED files can be kept on the device: detection_arena.py): a 1920 x 1440 frame is 8 MB, the train set would need terabytes, and every epoch crops
another part of the frame.  Measured: the launch takes 0.1 ms for 80 frames of 1440 x 1920, their
upload 11.6 ms, their Pillow decode 658 ms of one host core -- the workers' JPEG decode is what bounds this loader.

Over `ObjectronFrames(decode='device')` (dataloaders/jpeg.py) the workers return file bytes instead (`collate_jpeg`); `finish`
then uploads the bytes, puts the batch's index rows into the one pinned copy, allocates the packed frame buffer on the device,
copies the frames of files the index keeps on the host into their slots and calls `t3d_jpeg_decode_u8` on the same stream in
front of the augment launch.  The frame table comes from the index; prefetch, staging rotation, keys and the yielded tuple are
the same, and so are the batches, bit for bit.  `last_status` is the device status vector of the last decode call.
"""
import numpy as np
import torch

from .. import _native as N
from .detection import collate_frames, resize_boxes
from .jpeg import collate_jpeg, launch_decode, plan_batch
from .objectron import resize_records
from .staging import StagedLoader, upload

__all__ = ['GpuDetectionLoader']


class GpuDetectionLoader(StagedLoader):
    def __init__(self, dataset, pipeline, batch_size, sampler=None, shuffle=False, num_workers=0, drop_last=False, seed=0,
                 rank=0, prefetch=1):
        super().__init__(prefetch, min_staging=1 << 16)
        self.pipeline, self.seed, self.rank = pipeline, int(seed), int(rank)
        # ObjectronFrames(decode='device') -- directly or under a Subset: byte items, decoded in `finish` (dataloaders/jpeg.py)
        self._frames = getattr(dataset, 'dataset', dataset)
        self.decode = getattr(self._frames, 'decode', 'host')
        self.last_status = None         # device int32 [files decoded on the device] of the last batch's t3d_jpeg_decode_u8
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler,
                                                  shuffle=shuffle if sampler is None else False,
                                                  num_workers=int(num_workers or 0),
                                                  collate_fn=collate_jpeg if self.decode == 'device' else collate_frames,
                                                  pin_memory=torch.cuda.is_available(), drop_last=drop_last)
        self.dataset, self.batch_size = dataset, batch_size

    @property
    def sampler(self):
        return self.loader.sampler

    def __len__(self):
        return len(self.loader)

    def host_batch(self, host_batch, key_tail):
        """The host half of `finish`: draws, boxes and records of one collated batch.
        -> (rec [B] structured, gt_boxes f32 [B, G, 4], gt_labels i32 [B, G], gt_counts i32 [B], ori_shapes i32 [B, 2])."""
        _, desc, boxes, labels, counts = host_batch
        dnp, cnt = desc.numpy(), counts.numpy()
        B = len(dnp)
        cuts = np.cumsum(cnt)[:-1]
        bl, ll = np.split(boxes.numpy(), cuts), np.split(labels.numpy(), cuts)
        if self.pipeline.random:
            epoch = int(getattr(self.loader.sampler, 'epoch', 0))
            prm = self.pipeline.draw(B, (self.seed, epoch, self.rank) + tuple(key_tail))
            bl, ll = self.pipeline.boxes(bl, ll, dnp, prm)
            rec = self.pipeline.records(dnp, prm)
        else:
            rec = resize_records(dnp)
            row = np.repeat(np.arange(B), cnt)
            bl = np.split(resize_boxes(boxes.numpy(), row, dnp[:, 1], dnp[:, 2], self.pipeline.size), cuts)
        G = max([len(l) for l in ll] + [1])
        gb, gl = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32)
        gc = np.asarray([len(l) for l in ll], np.int32)
        for i in range(B):
            gb[i, :gc[i]], gl[i, :gc[i]] = bl[i], ll[i]
        return rec, gb, gl, gc, dnp[:, 1:].astype(np.int32)

    def finish(self, host_batch, key_tail, prefetch=None):
        """One host batch -> the device tuple, enqueued on the copy stream (prefetch >= 1: the ready event is appended) or on
        the current stream (prefetch 0)."""
        return self._public(*self._finish(host_batch, key_tail, prefetch))

    def _finish(self, host_batch, key_tail, prefetch=None):
        """-> (the device tuple, ready event or None)."""
        prefetch = self.prefetch if prefetch is None else prefetch
        packed, plan, fallback = host_batch[0], None, ()
        if self.decode == 'device':
            # byte items: the frame table comes from the index, the frames themselves are decoded below, on the device
            table, index = host_batch[1].numpy(), self._frames.index
            on_dev = np.flatnonzero(table[:, 1] == 0)
            desc = np.zeros((len(table), 3), np.int64)
            desc[:, 1:] = table[:, 3:5]
            desc[on_dev, 1], desc[on_dev, 2] = index.infos['h'][table[on_dev, 0]], index.infos['w'][table[on_dev, 0]]
            frame_bytes = desc[:, 1] * desc[:, 2] * 3
            desc[:, 0] = np.cumsum(frame_bytes) - frame_bytes              # the layout collate_frames packs
            if len(on_dev):
                plan = plan_batch([index.rows(int(i)) for i in table[on_dev, 0]], table[on_dev, 2], table[on_dev, 3], desc[on_dev, 0])
            fallback = [(int(table[k, 2]), int(desc[k, 0]), int(frame_bytes[k])) for k in np.flatnonzero(table[:, 1] == 1)]
            host_batch = (packed, torch.from_numpy(desc)) + tuple(host_batch[2:])
        rec, gb, gl, gc, shapes = self.host_batch(host_batch, key_tail)
        B, G = gb.shape[:2]
        oh, ow = self.pipeline.size
        parts = [rec.view(np.uint8), gb.reshape(-1).view(np.uint8), gl.reshape(-1).view(np.uint8), gc.view(np.uint8),
                 shapes.reshape(-1).view(np.uint8)]
        if plan is not None:                   # the batch's index rows ride in the same pinned copy
            parts += [plan['infos'].view(np.uint8), plan['segs'].view(np.uint8), plan['items'].view(np.uint8)]
        dev = torch.device('cuda', torch.cuda.current_device())
        stream = self._stream(dev, prefetch)
        up = upload(self._ring, parts, stream, dev)
        with torch.cuda.stream(stream):
            imgs = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=dev)
            src = packed.to(dev, non_blocking=True)
            if self.decode == 'device':
                raw, src = src, torch.empty(max(int(frame_bytes.sum()), 1), dtype=torch.uint8, device=dev)
                for at, to, n in fallback:     # frames the host had to decode go to their slots as they are
                    src[to:to + n].copy_(raw[at:at + n], non_blocking=True)
                if plan is not None:
                    self.last_status = launch_decode(raw, *[up.part(k, torch.uint8, -1) for k in (5, 6, 7)], plan, src)
            N.call('t3d_detect_augment_u8' if self.pipeline.random else 't3d_augment_crops_u8', N.ptr(src), src.numel(),
                   N.ptr(up.part(0, torch.uint8, -1)), N.ptr(imgs), B, oh, ow, N.stream())
        out = (imgs, up.part(1, torch.float32, B, G, 4), up.part(2, torch.int32, B, G), up.part(3, torch.int32, B))
        if not self.pipeline.random:
            out += (up.part(4, torch.int32, B, 2),)
        return out, self._ready(stream, prefetch)

    def __iter__(self):
        yield from self._batches(iter(self.loader), self._finish)
