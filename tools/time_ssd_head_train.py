"""Training the SSD heads at the config's batch (B = 80 = samples_per_gpu, bf16 storage, random 300x300 frames, G = 8):
HIP-event medians of `SSD300.head_backward` (frozen backbone forward, train-mode heads, MultiBox loss, head backward) and of
`DetectorHeadTrainer.train_step` (the same + t3d_sgd_step + the repack), of their parts (`forward_taps` alone, one
t3d_ssd_head_bwd call alone), and beside them the same head forward + backward -- the four heads given the taps and the loss's
gradients, backbone and loss excluded -- written in torch ops on the device (conv2d / batch_norm / relu / matmul, autograd).
Appends the raw lines to profiles/ssd_head_train_times.jsonl.
Usage: python tools/time_ssd_head_train.py [--out profiles/ssd_head_train_times.jsonl]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchdet3d import _native as N  # noqa: E402
from torchdet3d.models.ssd import BRANCHES, SSD300, TAPS  # noqa: E402
from torchdet3d.trainer import DetectorHeadTrainer  # noqa: E402

B, G = 80, 8


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


def torch_ops_heads(det, taps, grads):
    """Forward + backward of the four heads in torch ops (storage dtype, NCHW views of the NHWC taps), given the loss's
    gradients at the head outputs: -> the parameter gradients and the two tap gradients."""
    params, outs, leaves = [], [], []
    for l, k in enumerate(TAPS):
        t, Bn, H, W, C = taps[k]
        x = t.view(Bn, H, W, C).permute(0, 3, 1, 2).detach().requires_grad_(True)
        leaves.append(x)
        for bi, br in enumerate(BRANCHES):
            p = f'bbox_head.{br}.{l}'
            q = [det.p[p + s].detach().to(t.dtype).requires_grad_(True) for s in ('.0.weight', '.1.weight', '.1.bias', '.3.weight', '.3.bias')]
            params += q
            y = F.conv2d(x, q[0], None, 1, 1, 1, C)
            z = F.relu(F.batch_norm(y, None, None, q[1], q[2], True, 0.1, 1e-5))
            o = F.conv2d(z, q[3], q[4]).permute(0, 2, 3, 1).reshape(Bn * H * W, -1)
            n = o.shape[1]
            outs.append((o * grads[l][bi][:, :n].to(o.dtype)).sum())
    torch.stack(outs).sum().backward()
    return [q.grad for q in params], [x.grad for x in leaves]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssd_head_train_times.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the timing needs the GPU'
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (B, 300, 300, 3), dtype=torch.uint8, generator=g).to(dev)
    xy, wh = torch.rand(B, G, 2, generator=g) * 180 + 10, torch.rand(B, G, 2, generator=g) * 90 + 30
    gt = (torch.cat([xy, xy + wh], -1).float().to(dev), torch.randint(0, 9, (B, G), generator=g, dtype=torch.int32).to(dev),
          torch.randint(1, G + 1, (B,), generator=g, dtype=torch.int32).to(dev))
    det = SSD300(device=dev, dtype=torch.bfloat16)
    tr = DetectorHeadTrainer(det)
    r = det.head_backward(imgs, *gt, tap_grads=True)
    torch.cuda.synchronize()
    grads = [(a.clone(), b.clone()) for a, b in r['grads']]
    taps = det.backbone.forward_taps(imgs, TAPS)
    # the 1x1 half alone: the call head_backward makes, on its own buffers
    s = det._train[B]
    dout = s['P'](*[grads[h['l']][BRANCHES.index(h['br'])].data_ptr() for h in s['heads']])
    a, pt = ctypes.addressof, s['ptrs']

    def half():
        N.call('t3d_zero_batched', N.ptr(s['zero']), 1, N.stream())
        N.call('t3d_ssd_head_bwd', det.dt, len(s['heads']), a(dout), a(pt['y']), a(pt['scale']), a(pt['shift']), a(pt['w']),
               *[a(x) for x in s['geo']], N.ACT['relu'], a(pt['g']), a(pt['stats']), a(pt['dW']), a(pt['dbias']), N.ptr(s['work']),
               s['nb'], N.stream())
    # agreement of the torch form with the product on this batch (bf16 arithmetic in torch: a coarse figure, recorded)
    pg, tg = torch_ops_heads(det, taps, grads)
    torch.cuda.synchronize()
    keys = [f'bbox_head.{br}.{l}{sfx}' for l in range(len(TAPS)) for br in BRANCHES for sfx in ('.0.weight', '.1.weight', '.1.bias', '.3.weight', '.3.bias')]
    rel = max(float((det.hg[k].float() - q.float().view(det.hg[k].shape)).abs().max() / det.hg[k].abs().max().clamp(min=1e-30)) for k, q in zip(keys, pg))
    rows = []
    for what, fn, n in (('head_backward', lambda: det.head_backward(imgs, *gt), 30),
                        ('head_backward_tap_grads', lambda: det.head_backward(imgs, *gt, tap_grads=True), 30),
                        ('train_step', lambda: tr.train_step(imgs, *gt), 30),
                        ('forward_taps', lambda: det.backbone.forward_taps(imgs, TAPS), 30),
                        ('t3d_ssd_head_bwd', half, 30),
                        ('torch_ops_heads_fwd_bwd', lambda: torch_ops_heads(det, taps, grads), 10)):
        med, lo, hi, n = median_ms(fn, n=n)
        rows.append(dict(what=what, B=B, G=G, dtype='bf16', median_us=round(med * 1e3, 1), min_us=round(lo * 1e3, 1),
                         max_us=round(hi * 1e3, 1), runs=n, timer='HIP events around the call, host enqueue included',
                         torch_ops_max_rel_diff=rel, device=torch.cuda.get_device_name(0)))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for r_ in rows:
            f.write(json.dumps(r_) + '\n')


if __name__ == '__main__':
    main()
