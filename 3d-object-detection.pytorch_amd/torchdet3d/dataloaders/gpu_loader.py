"""Batches of Objectron crops finished on the GPU: the loader `build_loader` serves for a real data root.

A DataLoader (workers, pinned memory) yields the host side of a batch -- crops packed in one buffer plus a descriptor
table (`collate_crops`).  For each batch the main process draws the augmentation parameters, builds the kernel records and
the keypoints, uploads, and launches `t3d_augment_crops_u8` once (a pipeline with random_rescale, hue_saturation_value or
color_jitter: `t3d_augment_chain_crops_u8`, with a second record per sample in the same upload).  With `prefetch` >= 1 that work runs on a copy stream
`prefetch` batches ahead of the consumer, and each batch is handed over with an event the consumer's stream waits on, so
batch i + 1 is uploaded and augmented while step i runs.  `prefetch = 0` does it synchronously on the consumer's stream.

Yields device tensors `(imgs uint8 [B, oh, ow, 3], keypoints float32 [B, 9, 2], classes int64 [B])`: `Trainer.train`,
`Evaluator.val` and the step plan take them as they are.  The yielded tensors belong to the consumer (fresh allocations,
recorded on the consumer's stream); the pinned staging of the records, the one packed upload, the copy stream and the prefetch
loop are `StagedLoader`'s (staging.py).

`cache='device'` (`cfg.data.cache`): the pipeline resizes first, so resize(crop(frame)) is the same [oh, ow, 3] image in
every epoch.  One pass over the dataset (`fill_cache`, run at the first `__iter__`) decodes every object once and stores that
image -- `t3d_augment_crops_u8` with no flag set -- in an arena in device memory, slot i for dataset index i, with the
keypoints, the crop size and the class of every index on the host.  After it an epoch walks `loader.batch_sampler` (the
same batches, sharding and `set_epoch`), draws the same parameters with the same keys and launches
`t3d_augment_resized_u8` over the arena: no worker, no decode, no upload of pixels, and batches equal to the uncached
loader's bit for bit.  The arena must fit `cache_max_gb`; there is no partial cache.
"""
import numpy as np
import torch

from .. import _native as N
from .objectron import chain_scratch_bytes, chain_stages, collate_crops, resize_records
from .staging import StagedLoader, upload

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


class GpuAugmentLoader(StagedLoader):
    def __init__(self, dataset, pipeline, batch_size, sampler=None, shuffle=False, num_workers=0, drop_last=False, seed=0,
                 rank=0, prefetch=1, cache=None, cache_max_gb=32):
        super().__init__(prefetch, min_staging=1 << 16)
        self.pipeline, self.seed, self.rank = pipeline, int(seed), int(rank)
        self.cache = cache or None
        if self.cache is not None:
            if self.cache != 'device':
                raise ValueError(f"data.cache = {cache!r}: only 'device' (resized crops kept in GPU memory) or nothing is built")
            oh, ow = pipeline.size
            need, budget = len(dataset) * oh * ow * 3, int(float(cache_max_gb) * 2 ** 30)
            if need > budget:
                raise ValueError(f'data.cache: {len(dataset)} crops of {oh}x{ow}x3 need {need} bytes ({need / 2 ** 30:.3f} GiB), '
                                 f'over the budget data.cache_max_gb = {cache_max_gb} ({budget} bytes); there is no partial cache')
            self._arena = None                                 # uint8 [len(dataset) * oh * ow * 3] on the device (fill_cache)
            self._c_kp = self._c_desc = self._c_cats = None    # per index: keypoints f64 [N,9,2], (0, h, w) i64 [N,3], class i64 [N]
        self._num_workers = int(num_workers or 0)
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler,
                                                  shuffle=shuffle if sampler is None else False,
                                                  num_workers=int(num_workers or 0), collate_fn=collate_crops,
                                                  pin_memory=torch.cuda.is_available(), drop_last=drop_last)
        self.dataset = _FinishedDataset(dataset, self)
        self.batch_size = batch_size

    @property
    def sampler(self):
        return self.loader.sampler

    def __len__(self):
        return len(self.loader)

    def finish(self, host_batch, key_tail, prefetch=None):
        """One host batch -> device (imgs, keypoints, classes), enqueued on the copy stream (prefetch >= 1, with an event the
        caller hands to its consumer) or on the current stream (prefetch 0).  -> (imgs, kp, cats[, ready event])."""
        return self._public(*self._finish_batch(host_batch, key_tail, prefetch))

    def finish_cached(self, indices, key_tail, prefetch=None):
        """`finish` for a batch of dataset indices whose resized crops are in the arena."""
        return self._public(*self._finish_indices(indices, key_tail, prefetch))

    def _finish_batch(self, host_batch, key_tail, prefetch=None):
        packed, desc, kp64, cats = host_batch
        dnp = desc.numpy()
        return self._finish(packed, dnp, dnp, kp64.numpy(), cats.numpy(), key_tail, prefetch)

    def _finish_indices(self, indices, key_tail, prefetch=None):
        idx = np.asarray(indices, np.int64)
        oh, ow = self.pipeline.size
        where = np.stack([idx * (oh * ow * 3), np.full_like(idx, oh), np.full_like(idx, ow)], 1)     # (slot offset, oh, ow)
        return self._finish(None, where, self._c_desc[idx], self._c_kp[idx], self._c_cats[idx], key_tail, prefetch)

    def _finish(self, packed, where, dnp, kp64, cats, key_tail, prefetch):
        """where [B, 3]: (offset, h, w) of the kernel's source images (the packed crops, or arena slots when `packed` is
        None); dnp [B, 3]: the real crop sizes, which scale the keypoints.  -> ((imgs, kp, cats), ready event or None)."""
        prefetch = self.prefetch if prefetch is None else prefetch
        B = int(where.shape[0])
        oh, ow = self.pipeline.size
        epoch = int(getattr(self.loader.sampler, 'epoch', 0))
        prm = self.pipeline.draw(B, (self.seed, epoch, self.rank) + tuple(key_tail))
        rec = self.pipeline.records(where, prm)
        ext = None
        if self.pipeline.chained:
            rec, ext = rec
        kp = self.pipeline.keypoints(kp64, dnp, prm)
        # one pinned upload for records | keypoints | classes [| chain records]
        parts = [rec.view(np.uint8), kp.reshape(-1).view(np.uint8), cats.astype(np.int64).view(np.uint8)]
        if ext is not None:
            parts.append(ext.view(np.uint8))
        dev = torch.device('cuda', torch.cuda.current_device())
        stream = self._stream(dev, prefetch)
        up = upload(self._ring, parts, stream, dev)
        with torch.cuda.stream(stream):
            recd = up.part(0, torch.uint8, -1)
            imgs = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=dev)
            src = self._arena if packed is None else packed.to(dev, non_blocking=True)
            if ext is None:
                N.call('t3d_augment_resized_u8' if packed is None else 't3d_augment_crops_u8', N.ptr(src), src.numel(),
                       N.ptr(recd), N.ptr(imgs), B, oh, ow, N.stream())
            elif B:
                stages = chain_stages(rec, ext)
                scratch = torch.empty(max(chain_scratch_bytes(B, oh, ow, stages), 8), dtype=torch.uint8, device=dev)
                N.call('t3d_augment_chain_resized_u8' if packed is None else 't3d_augment_chain_crops_u8', N.ptr(src),
                       src.numel(), N.ptr(recd), N.ptr(up.part(3, torch.uint8, -1)), N.ptr(scratch), scratch.numel(),
                       N.ptr(imgs), B, oh, ow, stages, N.stream())
        return (imgs, up.part(1, torch.float32, B, 9, 2), up.part(2, torch.int64, B)), self._ready(stream, prefetch)

    def fill_cache(self):
        """The one decode pass: every dataset index, in order, through a DataLoader with the configured workers; its resized
        crop goes into arena slot `index`.  The workers exit with the pass.  Idempotent."""
        if self.cache is None:
            raise RuntimeError("fill_cache() needs a loader built with cache='device'")
        if self._arena is not None:
            return
        ds, (oh, ow) = self.dataset.host, self.pipeline.size
        n, slot = len(ds), oh * ow * 3
        dev = torch.device('cuda', torch.cuda.current_device())
        arena = torch.empty(max(n * slot, 1), dtype=torch.uint8, device=dev)
        c_kp, c_desc, c_cats = np.zeros((n, 9, 2), np.float64), np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
        it = iter(torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=False, num_workers=self._num_workers,
                                              collate_fn=collate_crops, pin_memory=True))
        i0 = 0
        for packed, desc, kp64, cats in it:
            B = int(desc.shape[0])
            dnp = desc.numpy()
            recd = torch.from_numpy(resize_records(dnp).view(np.uint8)).to(dev)
            src = packed.to(dev, non_blocking=True)
            out = arena[i0 * slot:(i0 + B) * slot]
            if out.data_ptr() & 3:                             # the kernel stores dwords: an odd slot goes through a staging tensor
                stage = torch.empty(B * slot, dtype=torch.uint8, device=dev)
                N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(recd), N.ptr(stage), B, oh, ow, N.stream())
                out.copy_(stage)
            else:
                N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(recd), N.ptr(out), B, oh, ow, N.stream())
            c_kp[i0:i0 + B], c_cats[i0:i0 + B] = kp64.numpy(), cats.numpy()
            c_desc[i0:i0 + B, 1:] = dnp[:, 1:]
            i0 += B
        del it                                                 # (the workers of a non-persistent DataLoader end with its iterator)
        if i0 != n:
            raise RuntimeError(f'fill_cache: the dataset yielded {i0} of {n} items')
        torch.cuda.current_stream(dev).synchronize()           # epochs read the arena on the copy stream
        self._arena, self._c_kp, self._c_desc, self._c_cats = arena, c_kp, c_desc, c_cats

    def __iter__(self):
        if self.cache is not None:
            self.fill_cache()
            yield from self._batches(iter(self.loader.batch_sampler), self._finish_indices)
        else:
            yield from self._batches(iter(self.loader), self._finish_batch)
