"""Batches of Objectron crops finished on the GPU: the loader `build_loader` serves for a real data root.

A DataLoader (workers, pinned memory) yields the host side of a batch -- crops packed in one buffer plus a descriptor
table (`collate_crops`).  For each batch the main process draws the augmentation parameters, builds the kernel records and
the keypoints, uploads, and launches `t3d_augment_crops_u8` once.  With `prefetch` >= 1 that work runs on a copy stream
`prefetch` batches ahead of the consumer, and each batch is handed over with an event the consumer's stream waits on, so
batch i + 1 is uploaded and augmented while step i runs.  `prefetch = 0` does it synchronously on the consumer's stream.

Yields device tensors `(imgs uint8 [B, oh, ow, 3], keypoints float32 [B, 9, 2], classes int64 [B])`: `Trainer.train`,
`Evaluator.val` and the step plan take them as they are.  The yielded tensors belong to the consumer (fresh allocations,
recorded on the consumer's stream); only the pinned staging of the records rotates, each buffer guarded by the event of its
last upload (the rule FrameCropper follows).
"""
import collections

import numpy as np
import torch

from .. import _native as N
from .objectron import collate_crops

__all__ = ['GpuAugmentLoader']


class _FinishedDataset:
    """`loader.dataset`: the host dataset, with each item finished on the GPU (a batch of one).  A test-mode item is the
    reference's 5-tuple (frame, image, keypoints, class, crop_cords), as Evaluator.visual_test reads it."""

    def __init__(self, dataset, loader):
        self.host, self._loader = dataset, loader

    def __len__(self):
        return len(self.host)

    def __getattr__(self, k):
        return getattr(self.__dict__['host'], k)

    def __getitem__(self, i):
        item = self.host[i]
        imgs, kp, cats = self._loader.finish(collate_crops([item]), key_tail=(0, int(i) + 1), prefetch=0)
        if len(item) == 5:
            return item[0], imgs[0], kp[0], int(cats[0]), item[4]
        return imgs[0], kp[0], int(cats[0])


class GpuAugmentLoader:
    NBUF = 3            # pinned record buffers in rotation

    def __init__(self, dataset, pipeline, batch_size, sampler=None, shuffle=False, num_workers=0, drop_last=False, seed=0,
                 rank=0, prefetch=1):
        self.pipeline, self.seed, self.rank, self.prefetch = pipeline, int(seed), int(rank), int(prefetch)
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler,
                                                  shuffle=shuffle if sampler is None else False,
                                                  num_workers=int(num_workers or 0), collate_fn=collate_crops,
                                                  pin_memory=torch.cuda.is_available(), drop_last=drop_last)
        self.dataset = _FinishedDataset(dataset, self)
        self.batch_size = batch_size
        self._slots = [[None, None] for _ in range(self.NBUF)]     # (pinned host buffer, event after its upload)
        self._turn = 0
        self._copy_stream = None

    @property
    def sampler(self):
        return self.loader.sampler

    def __len__(self):
        return len(self.loader)

    def _staging(self, nbytes):
        slot = self._slots[self._turn]
        self._turn = (self._turn + 1) % self.NBUF
        if slot[1] is not None:
            slot[1].synchronize()                  # the upload that last read this buffer has completed
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        return slot

    def finish(self, host_batch, key_tail, prefetch=None):
        """One host batch -> device (imgs, keypoints, classes), enqueued on the copy stream (prefetch >= 1, with an event the
        caller hands to its consumer) or on the current stream (prefetch 0).  -> (imgs, kp, cats[, ready event])."""
        prefetch = self.prefetch if prefetch is None else prefetch
        packed, desc, kp64, cats = host_batch
        B = int(desc.shape[0])
        oh, ow = self.pipeline.size
        epoch = int(getattr(self.loader.sampler, 'epoch', 0))
        dnp = desc.numpy()
        prm = self.pipeline.draw(B, (self.seed, epoch, self.rank) + tuple(key_tail))
        rec = self.pipeline.records(dnp, prm)
        kp = self.pipeline.keypoints(kp64.numpy(), dnp, prm)
        # one pinned upload for records | keypoints | classes (each part 8-byte aligned)
        nrec, nkp = B * rec.dtype.itemsize, B * 18 * 4
        nkp8 = (nkp + 7) // 8 * 8
        total = nrec + nkp8 + B * 8
        slot = self._staging(total)
        host = slot[0]
        host[:nrec].numpy()[...] = rec.view(np.uint8)
        host[nrec:nrec + nkp].numpy()[...] = kp.reshape(-1).view(np.uint8)
        host[nrec + nkp8:total].numpy()[...] = cats.numpy().astype(np.int64).view(np.uint8)
        dev = torch.device('cuda', torch.cuda.current_device())
        stream = torch.cuda.current_stream(dev)
        if prefetch > 0:
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=dev)
            stream = self._copy_stream
        with torch.cuda.stream(stream):
            meta = torch.empty(total, dtype=torch.uint8, device=dev)
            meta.copy_(host[:total], non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(stream)
            src = packed.to(dev, non_blocking=True)
            imgs = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=dev)
            N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(meta), N.ptr(imgs), B, oh, ow, N.stream())
            kp_d = meta[nrec:nrec + nkp].view(torch.float32).view(B, 9, 2)
            cats_d = meta[nrec + nkp8:total].view(torch.int64)
        if prefetch > 0:
            ready = torch.cuda.Event()
            ready.record(stream)
            return imgs, kp_d, cats_d, ready
        return imgs, kp_d, cats_d

    def __iter__(self):
        it = iter(self.loader)
        pending, done, b = collections.deque(), False, 0
        while True:
            while not done and len(pending) <= self.prefetch:
                try:
                    hb = next(it)
                except StopIteration:
                    done = True
                    break
                pending.append(self.finish(hb, (b,)))
                b += 1
            if not pending:
                return
            out = pending.popleft()
            if self.prefetch > 0:
                imgs, kp, cats, ready = out
                consumer = torch.cuda.current_stream(imgs.device)
                consumer.wait_event(ready)
                for t in (imgs, kp):             # (kp and cats share one allocation)
                    t.record_stream(consumer)
                out = (imgs, kp, cats)
            yield out
