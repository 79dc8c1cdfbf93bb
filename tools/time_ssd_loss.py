"""The SSD MultiBox loss at the config's batch (B = 80 = samples_per_gpu, G = 8, the 2044 real anchors, bf16 head outputs in the
head's padded rows): HIP-event median of `MultiBoxLoss.from_heads` (t3d_ssd_multibox_loss: two launches) with losses only and
with gradients, beside the same arithmetic written in torch ops on the device (a per-image loop with topk, as mmdet's
SSDHead.loss is written).  Appends the raw lines to profiles/ssd_multibox_loss_times.jsonl.
Usage: python tools/time_ssd_loss.py [--out profiles/ssd_multibox_loss_times.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402

import ssd_loss_ref as R  # noqa: E402
from torchdet3d.losses import MultiBoxLoss  # noqa: E402

B, G, NC = 80, 8, 9
HWS, NAS, CLS_STRIDES, REG_STRIDES = (361, 100), (4, 6), (40, 64), (16, 24)


def torch_ops_loss(cls, reg, anchors, gt_boxes, gt_labels, gt_counts, with_grads):
    """The same definition in torch ops on the device (dense fp32 tensors): IoU matrix, assignment, cross-entropy, a topk per
    image, smooth L1; the gradients by autograd."""
    Bn, A = cls.shape[0], anchors.shape[0]
    if with_grads:
        cls, reg = cls.detach().requires_grad_(True), reg.detach().requires_grad_(True)
    stds = torch.tensor(R.STDS, device=cls.device)
    sum_cls, sum_box, npos_all = [], [], []
    for b in range(Bn):
        n = int(gt_counts[b])                                   # (a host read per image, as in the torch original)
        g, gl = gt_boxes[b, :n], gt_labels[b, :n].long()
        label = torch.full((A,), NC, dtype=torch.long, device=cls.device)
        pos = torch.zeros(A, dtype=torch.bool, device=cls.device)
        if n:
            lt, rb = torch.maximum(g[:, None, :2], anchors[None, :, :2]), torch.minimum(g[:, None, 2:], anchors[None, :, 2:])
            wh = (rb - lt).clamp(min=0)
            inter = wh[..., 0] * wh[..., 1]
            ag, aa = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
            iou = inter / (ag[:, None] + aa[None] - inter).clamp(min=1e-6)
            m, arg = iou.max(0)
            asg = torch.where(m >= 0.4, arg, torch.full_like(arg, -1))
            asg[iou.argmax(1)] = torch.arange(n, device=cls.device)
            pos = asg >= 0
            label = torch.where(pos, gl[asg.clamp(min=0)], label)
        ce = torch.nn.functional.cross_entropy(cls[b], label, reduction='none')
        npos = pos.sum()
        k = int(min(3 * int(npos), A - int(npos)))
        idx = ce.detach().masked_fill(pos, -1.0).topk(k).indices
        sum_cls.append(ce[pos].sum() + ce[idx].sum())
        if n and int(npos):
            a, gg = anchors[pos], g[asg[pos]]
            pw, ph, gw, gh = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], gg[:, 2] - gg[:, 0], gg[:, 3] - gg[:, 1]
            t = torch.stack([((gg[:, 0] + gg[:, 2]) * 0.5 - (a[:, 0] + a[:, 2]) * 0.5) / pw, ((gg[:, 1] + gg[:, 3]) * 0.5 - (a[:, 1] + a[:, 3]) * 0.5) / ph,
                             torch.log(gw / pw), torch.log(gh / ph)], -1) / stds
            sum_box.append(torch.nn.functional.smooth_l1_loss(reg[b][pos], t, reduction='sum', beta=1.0))
        npos_all.append(npos)
    avg = torch.stack(npos_all).sum().clamp(min=1)
    lc, lb = torch.stack(sum_cls).sum() / avg, (torch.stack(sum_box).sum() if sum_box else cls.new_zeros(())) / avg
    if with_grads:
        (lc + lb).backward()
    return lc, lb


def median_ms(fn, warm=5, n=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.asarray(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max()), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssd_multibox_loss_times.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the timing needs the GPU'
    rng = np.random.default_rng(0)
    A = 2044
    cls = (rng.standard_normal((B, A, NC + 1)) * 2).astype(np.float32)
    reg = rng.standard_normal((B, A, 4)).astype(np.float32)
    gb, gl = R._random_gt(rng, B, G)
    gc = rng.integers(1, G + 1, B).astype(np.int32)
    dev = 'cuda:0'
    anchors = torch.from_numpy(R.real_anchors()).to(dev)
    outs = [(torch.from_numpy(c).to(dev).to(torch.bfloat16), torch.from_numpy(r).to(dev).to(torch.bfloat16), hw)
            for c, r, hw in zip(R.to_levels(cls, HWS, NAS, NC + 1, CLS_STRIDES, pad=0.0), R.to_levels(reg, HWS, NAS, 4, REG_STRIDES, pad=0.0), HWS)]
    gt = [torch.from_numpy(x).to(dev) for x in (gb, gl, gc)]
    mb = MultiBoxLoss(anchors)
    # the torch form gets the same (bf16-rounded) values as dense fp32 tensors
    cls_d = torch.from_numpy(cls).to(dev).to(torch.bfloat16).float()
    reg_d = torch.from_numpy(reg).to(dev).to(torch.bfloat16).float()
    rows = []
    for with_grads in (False, True):
        r = mb.from_heads(outs, *gt, with_grads=with_grads, nanchors=list(NAS))
        lc, lb = torch_ops_loss(cls_d, reg_d, anchors, *gt, with_grads)
        torch.cuda.synchronize()
        diff = (abs(r['loss_cls'].item() - lc.item()), abs(r['loss_bbox'].item() - lb.item()))
        for what, fn in (('t3d_ssd_multibox_loss', lambda: mb.from_heads(outs, *gt, with_grads=with_grads, nanchors=list(NAS))),
                         ('torch_ops', lambda: torch_ops_loss(cls_d, reg_d, anchors, *gt, with_grads))):
            med, lo, hi, n = median_ms(fn, n=30 if what != 'torch_ops' else 10)
            rows.append(dict(what=what, with_grads=with_grads, B=B, G=G, A=A, dtype='bf16' if what != 'torch_ops' else 'fp32',
                             median_us=round(med * 1e3, 1), min_us=round(lo * 1e3, 1), max_us=round(hi * 1e3, 1), runs=n,
                             timer='HIP events around the call (allocations of the outputs included)',
                             loss_cls=r['loss_cls'].item(), loss_bbox=r['loss_bbox'].item(), loss_diff_vs_torch_ops=diff,
                             device=torch.cuda.get_device_name(0)))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
