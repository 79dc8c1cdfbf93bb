"""Training the whole SSD detector at the config's batch (B = 80 = samples_per_gpu, bf16 storage, random 300x300 frames,
G = 8): HIP-event medians of `SSD300.train_backward` (train-mode tapped backbone, train-mode heads, MultiBox loss, head
backward, backbone backward) and of `DetectorTrainer.train_step` (the same + two t3d_sgd_step + the heads' repack; the engine's
own repack falls into the next step's forward), of the step's parts timed in place (events between the parts of one step:
train-mode backbone forward | heads + loss + head backward | backbone backward | the SGD calls and the heads' repack), and
beside them the frozen-backbone `DetectorHeadTrainer.train_step` on the same box and batch, and the regression network's
forward(train) + backward at a like pixel count (144 crops of 224x224 = 7.23 M pixels against 80 x 300 x 300 = 7.2 M) -- the
same blocks plus conv.0 / conv.1, the pool and the heads.
Appends the raw lines to profiles/detector_train_times.jsonl.
Usage: python tools/time_detector_train.py [--out profiles/detector_train_times.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402

from torchdet3d import _native as N  # noqa: E402
from torchdet3d.models.engine import Net  # noqa: E402
from torchdet3d.models.ssd import SSD300, TAPS  # noqa: E402
from torchdet3d.trainer import DetectorHeadTrainer, DetectorTrainer  # noqa: E402

B, G, RUNS = 80, 8, 30
PARTS = ('backbone_forward_train', 'heads_loss_head_backward', 'backbone_backward', 'sgd_and_head_repack')


def _stat(ms):
    ms = np.asarray(ms)
    return dict(median_us=round(float(np.median(ms)) * 1e3, 1), min_us=round(float(ms.min()) * 1e3, 1),
                max_us=round(float(ms.max()) * 1e3, 1), runs=len(ms))


def time_whole(fn, warm=5, n=RUNS):
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
    return _stat(ms)


def step_in_parts(det, tr, imgs, gt):
    """DetectorTrainer.train_step, its pieces called one by one with an event between them -> the four elapsed times (ms)."""
    bb = det.backbone
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    taps = bb.forward_taps_train(imgs, TAPS)
    ev[1].record()
    r = det._heads_fwd_bwd(taps, B, *gt, True)
    ev[2].record()
    bb.backward_taps(dict(zip(TAPS, r['dtaps'])))
    ev[3].record()
    lr, st = tr.lr_at(0, tr.it), N.stream()
    N.call('t3d_sgd_step', N.ptr(det.hflat), N.ptr(det.hgrad), N.ptr(tr.buf), det.hflat.numel(), lr, tr.momentum, tr.weight_decay,
           0, tr.it + 1, 1.0, st)
    N.call('t3d_sgd_step', N.ptr(bb.flat), N.ptr(bb.gflat), N.ptr(tr.bbuf), tr.nbackbone, lr, tr.momentum, tr.weight_decay,
           0, tr.it + 1, 1.0, st)
    tr.it += 1
    det.params_changed()
    det.repack_heads(B)
    bb._packed_dirty = True
    ev[4].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'detector_train_times.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the timing needs the GPU'
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (B, 300, 300, 3), dtype=torch.uint8, generator=g).to(dev)
    xy, wh = torch.rand(B, G, 2, generator=g) * 180 + 10, torch.rand(B, G, 2, generator=g) * 90 + 30
    gt = (torch.cat([xy, xy + wh], -1).float().to(dev), torch.randint(0, 9, (B, G), generator=g, dtype=torch.int32).to(dev),
          torch.randint(1, G + 1, (B,), generator=g, dtype=torch.int32).to(dev))
    rows = []

    def row(what, stat, **kw):
        rows.append(dict(what=what, B=B, G=G, dtype='bf16', **stat, timer='HIP events around the call, host enqueue included',
                         device=torch.cuda.get_device_name(0), **kw))
        print(json.dumps(rows[-1]), flush=True)

    # lr 0: thirty-five steps on one random batch must not walk the weights anywhere (the timings do not depend on the values)
    det = SSD300(device=dev, dtype=torch.bfloat16)
    row('train_backward', time_whole(lambda: det.train_backward(imgs, *gt)))
    tr = DetectorTrainer(det, lr=0.0)
    row('DetectorTrainer.train_step', time_whole(lambda: tr.train_step(imgs, *gt)))
    for _ in range(5):
        step_in_parts(det, tr, imgs, gt)
    parts = np.asarray([step_in_parts(det, tr, imgs, gt) for _ in range(RUNS)])
    for i, what in enumerate(PARTS):
        row('part:' + what, _stat(parts[:, i]), note='events between the parts of one train_step')
    row('part:sum_of_the_four', _stat(parts.sum(1)))
    assert not det.backbone.nonfinite()
    det2 = SSD300(device=dev, dtype=torch.bfloat16)
    trh = DetectorHeadTrainer(det2, lr=0.0)
    row('DetectorHeadTrainer.train_step', time_whole(lambda: trh.train_step(imgs, *gt)), note='frozen backbone')
    row('forward_taps', time_whole(lambda: det2.backbone.forward_taps(imgs, TAPS)), note='frozen backbone forward (inference mode)')
    # the regression network at a like pixel count: forward(train) + backward, loss excluded
    Br = 144
    net = Net('mobilenetv2', 9, dev, torch.bfloat16)
    crops = torch.randint(0, 256, (Br, 224, 224, 3), dtype=torch.uint8, generator=g).to(dev)
    cats = torch.randint(0, 9, (Br,), generator=g).to(dev)
    dkp, dlg = torch.randn(Br, 18, generator=g).to(dev) * 1e-3, torch.randn(Br, 9, generator=g).to(dev) * 1e-3

    def reg():
        net.forward(crops, cats, train=True)
        net.backward(dkp, dlg)
    row('regression_forward_train_backward', time_whole(reg), note=f'{Br} crops of 224x224 ({Br * 224 * 224} pixels against {B * 300 * 300})')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for r_ in rows:
            f.write(json.dumps(r_) + '\n')


if __name__ == '__main__':
    main()
