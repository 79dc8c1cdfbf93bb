"""Training of the SSD detector: the heads over a frozen backbone (`DetectorHeadTrainer`, piece (b1) of detector training;
models/ssd.py: `head_backward`) and heads and tapped backbone together (`DetectorTrainer`, piece (b2); `train_backward`).

The optimizer and schedule are the detector config's (`configs/detection/mnv2_ssd_300_2_heads.py:145-153` of the reference):
SGD(lr=0.05, momentum=0.9, weight_decay=5e-4), `optimizer_config = dict()` -- no gradient clipping --, and
lr_config(policy='step', warmup='linear', warmup_iters=1200, warmup_ratio=1/3, step=[25, 30, 35]) per mmcv's LrUpdaterHook.
One step is `head_backward` followed by ONE t3d_sgd_step over the heads' flat parameter buffer and one repack of the 1x1
weights; nothing is read back.  The loss is loss_cls + loss_bbox: the config's `loss_balancing` (the fork's own learnable
weighting, no published definition) stays unbuilt.  `DetectorTrainer` is the config as written (norm_eval=False,
frozen_stages=-1: one SGD over backbone and heads): `train_backward`, then t3d_sgd_step over the heads' buffer and over the
backbone's trained prefix of its flat buffer -- the stem and features.*, which come first in state-dict order; what the detector
does not use of the engine (conv.*, classifier.*, cls_fc.*, regressors.*) lies behind the prefix, has a zero gradient, and is
left alone: it must not decay.
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


class DetectorTrainer(DetectorHeadTrainer):
    """The detector config's training step on heads AND backbone: same SGD, same schedule, one more t3d_sgd_step."""

    def __init__(self, det, **kw):
        super().__init__(det, **kw)
        bb = det.backbone
        self.nbackbone = bb.offsets[bb.arch.keys.last_w][0]        # the stem and features.*: [0, offset of conv.0.weight)
        assert self.nbackbone % 4 == 0 and all(o >= self.nbackbone or o + n <= self.nbackbone for o, n in bb.offsets.values())
        self.bbuf = torch.zeros(self.nbackbone, device=bb.flat.device)     # the backbone's momentum buffer

    @torch.no_grad()
    def train_step(self, imgs, gt_boxes, gt_labels, gt_counts, epoch=0):
        """-> (loss_cls, loss_bbox, loss_cls + loss_bbox) as 0-dim device tensors of the batch BEFORE the update."""
        det, bb = self.det, self.det.backbone
        r = det.train_backward(imgs, gt_boxes, gt_labels, gt_counts)
        lr, st = self.lr_at(epoch, self.it), N.stream()
        N.call('t3d_sgd_step', N.ptr(det.hflat), N.ptr(det.hgrad), N.ptr(self.buf), det.hflat.numel(), lr, self.momentum,
               self.weight_decay, 0, self.it + 1, 1.0, st)
        N.call('t3d_sgd_step', N.ptr(bb.flat), N.ptr(bb.gflat), N.ptr(self.bbuf), self.nbackbone, lr, self.momentum,
               self.weight_decay, 0, self.it + 1, 1.0, st)
        self.it += 1
        det.params_changed()
        det.repack_heads(int(imgs.shape[0]))
        # written through a raw pointer: the engine repacks its storage-dtype weights at the start of its next pass
        torch.autograd.graph.increment_version(bb.flat)
        bb._packed_dirty = True
        return r['loss_cls'], r['loss_bbox'], r['loss_cls'] + r['loss_bbox']
