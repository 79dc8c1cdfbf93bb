"""Training of the SSD heads over a frozen backbone (piece (b1) of detector training; models/ssd.py: `head_backward`).

The optimizer and schedule are the detector config's (`configs/detection/mnv2_ssd_300_2_heads.py:145-153` of the reference):
SGD(lr=0.05, momentum=0.9, weight_decay=5e-4), `optimizer_config = dict()` -- no gradient clipping --, and
lr_config(policy='step', warmup='linear', warmup_iters=1200, warmup_ratio=1/3, step=[25, 30, 35]) per mmcv's LrUpdaterHook.
One step is `head_backward` followed by ONE t3d_sgd_step over the heads' flat parameter buffer and one repack of the 1x1
weights; nothing is read back.  The loss is loss_cls + loss_bbox: the config's `loss_balancing` (the fork's own learnable
weighting, no published definition) stays unbuilt.  The backbone is not trained here: that is piece (b2).
"""
import torch

from .. import _native as N


class DetectorHeadTrainer:
    def __init__(self, det, lr=0.05, momentum=0.9, weight_decay=5e-4, warmup_iters=1200, warmup_ratio=1 / 3, steps=(25, 30, 35),
                 gamma=0.1, print_freq=50):
        self.det = det
        self.lr, self.momentum, self.weight_decay = float(lr), float(momentum), float(weight_decay)
        self.warmup_iters, self.warmup_ratio = int(warmup_iters), float(warmup_ratio)
        self.steps, self.gamma, self.print_freq = tuple(int(s) for s in steps), float(gamma), int(print_freq)
        self.buf = torch.zeros_like(det.hflat)          # the momentum buffer
        self.it = 0                                     # iterations done (the warm-up counts them across epochs)

    def lr_at(self, epoch, it):
        """mmcv's step policy with linear warm-up, on the host in fp64: lr * gamma**(number of steps <= epoch), times
        1 - (1 - it / warmup_iters) * (1 - warmup_ratio) while it < warmup_iters (`it`: iterations since the start)."""
        reg = self.lr * self.gamma ** sum(1 for s in self.steps if s <= epoch)
        if it < self.warmup_iters:
            reg *= 1.0 - (1.0 - it / self.warmup_iters) * (1.0 - self.warmup_ratio)
        return reg

    @torch.no_grad()
    def train_step(self, imgs, gt_boxes, gt_labels, gt_counts, epoch=0):
        """-> (loss_cls, loss_bbox, loss_cls + loss_bbox) as 0-dim device tensors of the batch BEFORE the update."""
        det = self.det
        r = det.head_backward(imgs, gt_boxes, gt_labels, gt_counts)
        # coupled weight decay on every parameter, as mmdet's plain SGD (no paramwise_cfg)
        N.call('t3d_sgd_step', N.ptr(det.hflat), N.ptr(det.hgrad), N.ptr(self.buf), det.hflat.numel(), self.lr_at(epoch, self.it),
               self.momentum, self.weight_decay, 0, self.it + 1, 1.0, N.stream())
        self.it += 1
        det.params_changed()
        det.repack_heads(int(imgs.shape[0]))
        return r['loss_cls'], r['loss_bbox'], r['loss_cls'] + r['loss_bbox']

    def train(self, loader, epoch):
        """One epoch over a `GpuDetectionLoader`; the losses are read back every `print_freq` steps only."""
        if hasattr(getattr(loader, 'sampler', None), 'set_epoch'):
            loader.sampler.set_epoch(epoch)
        last = None
        for i, batch in enumerate(loader):
            last = self.train_step(*batch[:4], epoch=epoch)
            if (i + 1) % self.print_freq == 0:
                lc, lb, tot = (float(x) for x in last)
                print(f'epoch {epoch} iter {i + 1}/{len(loader)} lr {self.lr_at(epoch, self.it - 1):.5f} '
                      f'loss_cls {lc:.4f} loss_bbox {lb:.4f} loss {tot:.4f}')
        return None if last is None else tuple(float(x) for x in last)
