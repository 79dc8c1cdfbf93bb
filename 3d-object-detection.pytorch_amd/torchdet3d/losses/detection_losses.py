"""MultiBox training loss of the SSD detector on the device (csrc/ssd_loss.hip: t3d_ssd_multibox_loss).

The training half of the reference's detector config (`configs/detection/mnv2_ssd_300_2_heads.py:41-55`:
MaxIoUAssigner(pos_iou_thr=0.4, neg_iou_thr=0.4, min_pos_iou=0, gt_max_assign_all=False), smoothl1_beta=1, neg_pos_ratio=3)
per the published mmdet 2.x definitions (SSDHead.loss, MaxIoUAssigner, DeltaXYWHBBoxCoder, smooth_l1_loss); the implementing
fork is external to the reference, so parity with the reference's detector is unpinned -- include/t3d.h and
tests/ssd_loss_ref.py are the definition.  The config's `loss_balancing=True` is the fork's own learnable weighting, has no
published definition and is not built.

Device tensors only; there is no CPU fallback.  One call is two launches and synchronises nothing.
"""
import ctypes

import torch

from .. import _native as N

STDS = (0.1, 0.1, 0.2, 0.2)          # config :34 (the coder's target stds)


class MultiBoxLoss:
    """`from_heads`: the loss (and the gradients with respect to the head outputs) of `SSD300.head_outputs`' tensors;
    calling the object: the same entry point over dense fp32 tensors, as a `torch.autograd.Function`."""

    def __init__(self, anchors, num_classes=9, pos_iou_thr=.4, neg_iou_thr=.4, min_pos_iou=0., neg_pos_ratio=3,
                 smoothl1_beta=1., stds=STDS):
        anchors = torch.as_tensor(anchors)
        if not anchors.is_cuda:
            raise RuntimeError('MultiBoxLoss needs its anchors on the device (there is no CPU path)')
        self.anchors = anchors.to(torch.float32).contiguous().view(-1, 4)
        self.nc = int(num_classes)
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = float(pos_iou_thr), float(neg_iou_thr), float(min_pos_iou)
        self.neg_pos_ratio, self.beta = int(neg_pos_ratio), float(smoothl1_beta)
        self._stds = (ctypes.c_float * 4)(*[float(s) for s in stds])

    def _levels(self, outs, nanchors):
        A = self.anchors.shape[0]
        B = None
        for cls, reg, hw in outs:
            if cls.shape[0] % hw or reg.shape[0] != cls.shape[0]:
                raise RuntimeError('head outputs: rows are not B * hw')
            if B is not None and cls.shape[0] // hw != B:
                raise RuntimeError('head outputs: the levels disagree on the batch size')
            B = cls.shape[0] // hw
        if nanchors is None:
            if len(outs) == 1:
                nanchors = [A // outs[0][2]]
            else:       # (unpadded box channels are anchors * 4; the class channels may carry pad)
                nanchors = [min(reg.shape[1] // 4, cls.shape[1] // (self.nc + 1)) for cls, reg, _ in outs]
        if sum(o[2] * n for o, n in zip(outs, nanchors)) != A:
            raise RuntimeError(f'head outputs with {list(nanchors)} anchors per pixel do not make the {A} anchors; pass nanchors=')
        return B, [int(n) for n in nanchors]

    def from_heads(self, outs, gt_boxes, gt_labels, gt_counts, with_grads=True, nanchors=None):
        """outs: per level (cls [B*hw, cls_stride], reg [B*hw, reg_stride], hw) in one storage dtype (fp32 / bf16);
        gt_boxes [B,G,4] fp32, gt_labels [B,G] int32, gt_counts [B] int32 -> dict(loss_cls, loss_bbox: 0-dim fp64 device
        tensors; total_pos, total_mined likewise; num_pos [B] int32; assigned [B,A] int32: ground-truth index, -1 unused
        negative, -2 mined negative; grads: per level (dcls, dreg) fp32 in the rows and strides of the inputs, or None)."""
        outs = [(o[0], o[1], int(o[2])) for o in outs]
        nl = len(outs)
        B, nanchors = self._levels(outs, nanchors)
        dev = self.anchors.device
        A = self.anchors.shape[0]
        if gt_boxes.dtype != torch.float32 or gt_labels.dtype != torch.int32 or gt_counts.dtype != torch.int32:
            raise RuntimeError('gt_boxes is fp32, gt_labels and gt_counts are int32')
        if gt_boxes.shape[0] != B or gt_labels.shape[0] != B or gt_counts.shape[0] != B or gt_boxes.shape[1] != gt_labels.shape[1]:
            raise RuntimeError('ground truth: [B,G,4], [B,G], [B] expected')
        G = int(gt_boxes.shape[1])
        dt = N.dtype_code(outs[0][0])
        if dt == N.F16 or any(N.dtype_code(t) != dt for o in outs for t in o[:2]):
            raise RuntimeError('head outputs are fp32 or bf16, all alike')
        nb = N.lib().t3d_ssd_multibox_work_bytes(B, A)
        if nb < 0:
            raise RuntimeError(f't3d_ssd_multibox_work_bytes failed with code {nb}')
        work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        # (the two launches write every element of the three outputs; an empty batch launches nothing)
        alloc = torch.empty if B else torch.zeros
        scalars = alloc(4, dtype=torch.float64, device=dev)
        num_pos = alloc(B, dtype=torch.int32, device=dev)
        assigned = alloc((B, A), dtype=torch.int32, device=dev)
        grads = [(torch.empty(o[0].shape, dtype=torch.float32, device=dev), torch.empty(o[1].shape, dtype=torch.float32, device=dev))
                 for o in outs] if with_grads else None
        P, I = ctypes.c_void_p * nl, ctypes.c_int * nl
        # the per-level HOST arrays of the entry point (addresses: a recorded plan keeps them as they are)
        host = [P(*[o[0].data_ptr() for o in outs]), P(*[o[1].data_ptr() for o in outs]), I(*[o[2] for o in outs]),
                I(*nanchors), I(*[o[0].shape[1] for o in outs]), I(*[o[1].shape[1] for o in outs])]
        gh = [P(*[g[0].data_ptr() for g in grads]), P(*[g[1].data_ptr() for g in grads])] if with_grads else []
        if N.recorder is not None:
            N.recorder.keep += [host, gh, self._stds, outs, grads, work, scalars, num_pos, assigned, self.anchors, gt_boxes,
                                gt_labels, gt_counts]
        N.call('t3d_ssd_multibox_loss', dt, nl, *[ctypes.addressof(h) for h in host], N.ptr(self.anchors),
               N.ptr(gt_boxes) if G else None, N.ptr(gt_labels) if G else None, N.ptr(gt_counts), B, G, self.nc,
               self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou, self.neg_pos_ratio, self.beta,
               ctypes.addressof(self._stds), N.ptr(work), nb, N.ptr(scalars), N.ptr(num_pos), N.ptr(assigned),
               ctypes.addressof(gh[0]) if with_grads else None, ctypes.addressof(gh[1]) if with_grads else None, N.stream())
        return dict(loss_cls=scalars[0], loss_bbox=scalars[1], total_pos=scalars[2], total_mined=scalars[3],
                    num_pos=num_pos, assigned=assigned, grads=grads)

    def __call__(self, cls_score, bbox_pred, gt_boxes, gt_labels, gt_counts):
        """cls_score [B,A,nc+1], bbox_pred [B,A,4] dense fp32 -> (loss_cls, loss_bbox), differentiable with respect to both."""
        return _MultiBoxFn.apply(cls_score, bbox_pred, self, gt_boxes, gt_labels, gt_counts)


class _MultiBoxFn(torch.autograd.Function):
    """One level with hw = A and one anchor per pixel; the gradients come out of the forward's call and `backward` scales
    them by the incoming scalars."""

    @staticmethod
    def forward(ctx, cls_score, bbox_pred, mb, gt_boxes, gt_labels, gt_counts):
        B, A = cls_score.shape[0], cls_score.shape[1]
        if cls_score.dtype != torch.float32 or bbox_pred.dtype != torch.float32:
            raise RuntimeError('the dense form takes fp32 tensors')
        if tuple(cls_score.shape) != (B, A, mb.nc + 1) or tuple(bbox_pred.shape) != (B, A, 4) or A != mb.anchors.shape[0]:
            raise RuntimeError('cls_score [B,A,nc+1] and bbox_pred [B,A,4] over the loss\'s anchors expected')
        cls2 = cls_score.detach().contiguous().view(B * A, mb.nc + 1)
        reg2 = bbox_pred.detach().contiguous().view(B * A, 4)
        r = mb.from_heads([(cls2, reg2, A)], gt_boxes, gt_labels, gt_counts, with_grads=True, nanchors=[1])
        dcls, dreg = r['grads'][0]
        ctx.save_for_backward(dcls.view(B, A, mb.nc + 1), dreg.view(B, A, 4))
        return r['loss_cls'].clone(), r['loss_bbox'].clone()

    @staticmethod
    def backward(ctx, g_cls, g_bbox):
        dcls, dreg = ctx.saved_tensors
        return dcls * g_cls.to(torch.float32), dreg * g_bbox.to(torch.float32), None, None, None, None
