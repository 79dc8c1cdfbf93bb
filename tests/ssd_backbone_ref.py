"""Restatement of the detector's tapped backbone in TRAINING mode on the CPU: the definition tests/test_detector_train_host.py
and tests/test_gpu_detector_train.py hold `Net.forward_taps_train` / `Net.backward_taps`, `SSD300.train_backward` and
`DetectorTrainer` to.

The backbone is MobileNetV2's stem + features.1 .. features.17 (the detector config's `mobilenetv2_w1`, tapped after features.13
-- 96 channels, stride 16 -- and features.17 -- 320 channels, stride 32; `norm_eval=False, frozen_stages=-1`: every BatchNorm
normalises with its batch statistics and moves its running estimates).  It is assembled from the oracle's own pieces
(`oracle.model.block_forward`, `_bn`, `act_fn`); the gradients come from torch autograd of  sum_k <tap_k, cotangent_k>  in
float32 and in float64.  The head half is tests/ssd_head_ref.py (imported by the tests, not repeated here).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.model import _bn, act_fn, block_forward
from oracle.specs import arch
from oracle.weights import make_inputs, make_state_dict

NAME = 'mobilenetv2'
TAPS = (13, 17)
# the case of the GPU gradient test: small enough for a CPU float64 autograd, and well conditioned (test_detector_train_host.py)
CASE = dict(B=2, H=96, W=128, seed=0, cot_seed=0)
SCALE_FLOOR = 1e-3          # of the largest gradient over all tensors (tests/test_gpu_golden.py's floor)
# torch-CPU splits the sums of a convolution by thread count, and whether a ReLU6 kink of the float32 run flips against the
# float64 run depends on that order: with 2 .. 16 threads the case has no flip (worst spread 2.9e-4), with 1 or 32 it has one
# (4.4e-2).  The restatement therefore runs on a fixed count, as tests/test_oracle_golden.py's does, and restores the caller's.
REF_THREADS = 8


def trained_keys(sd):
    """Learnable entries of the tapped backbone (stem + features.*), in state-dict order."""
    return [k for k in sd if k.startswith('features.') and 'running' not in k and not k.endswith('num_batches_tracked')]


def forward_taps(sd, x, train=True, taps=TAPS):
    """sd: {key: tensor} of one dtype (BatchNorm buffers are updated IN PLACE when train), x [B,3,H,W] -> {k: [B,C,h,w]}."""
    a = arch(NAME)
    y = F.conv2d(x, sd['features.0.0.weight'], None, 2, 1)
    y = act_fn(_bn(sd, 'features.0.1', y, train), a['stem_act'])
    out = {}
    for i, blk in enumerate(a['blocks'][:max(taps)]):
        y = block_forward(sd, f'features.{i + 1}', blk, y, train)
        if i + 1 in taps:
            out[i + 1] = y
    return out


def rows(t):
    """[B,C,h,w] -> the engine's NHWC rows [B*h*w, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def tap_dims(B, H, W):
    """{tap: (B, h, w, C)} of a B x H x W input (3x3 convs of stride 2, pad 1: h -> (h + 1) // 2)."""
    a, out = arch(NAME), {}
    h, w = (H + 1) // 2, (W + 1) // 2
    for i, blk in enumerate(a['blocks'][:max(TAPS)]):
        if blk['s'] == 2:
            h, w = (h + 1) // 2, (w + 1) // 2
        if i + 1 in TAPS:
            out[i + 1] = (B, h, w, blk['cout'])
    return out


def stored(x, bf16):
    x = torch.as_tensor(x, dtype=torch.float32)
    return x.to(torch.bfloat16).to(torch.float32) if bf16 else x


def cotangents(dims, seed=0, bf16=False, zero=()):
    """{tap: [B*h*w, C] float32} seeded normal draws as the storage dtype holds them; taps in `zero` all zero."""
    g = torch.Generator().manual_seed(4242 + seed)
    out = {}
    for k in sorted(dims):
        B, h, w, C = dims[k]
        d = stored(torch.randn(B * h * w, C, generator=g), bf16)
        out[k] = torch.zeros_like(d) if k in zero else d
    return out


def grads(sd, imgs, cot, dtype):
    """Autograd of sum_k <tap_k rows, cot_k> in `dtype` ('float32' / 'float64') -> dict(grads {key: float64 numpy}, taps {k: rows,
    float64 numpy}, buffers {key: float64 numpy} after the pass).  `sd` is not modified."""
    dt = torch.float64 if dtype == 'float64' else torch.float32
    q = {}
    for k, v in sd.items():
        if not (k.startswith('features.')):
            continue
        if v.dtype.is_floating_point:
            q[k] = v.detach().to(dt).clone()
            if 'running' not in k:
                q[k].requires_grad_(True)
        else:
            q[k] = v.detach().clone()
    taps = forward_taps(q, imgs.to(dt), True, tuple(sorted(cot)))
    tot = sum((rows(taps[k]) * cot[k].to(dt)).sum() for k in cot)
    tot.backward()
    keys = trained_keys(q)
    return dict(grads={k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])).double().numpy() for k in keys},
                taps={k: rows(taps[k]).detach().double().numpy() for k in taps},
                buffers={k: v.detach().double().numpy() for k, v in q.items() if k not in keys})


def spreads(g32, g64):
    """{key: (spread, scale)}: largest |g32 - g64| of a tensor relative to scale = max(max|g64 of the tensor|, SCALE_FLOOR *
    max|g64 over all tensors|) -- a BatchNorm shift in front of a mean-subtracting BatchNorm has a true gradient of 0 and is
    judged against the overall gradient scale, not against its own round-off."""
    gmax = max(float(np.abs(v).max()) for v in g64.values())
    out = {}
    for k, v in g64.items():
        scale = max(float(np.abs(v).max()), SCALE_FLOOR * gmax)
        out[k] = (float(np.abs(g32[k] - v).max()) / scale, scale)
    return out


@functools.lru_cache(maxsize=None)
def case(zero=(), cot_seed=None):
    """The GPU gradient test's case, computed once and shared: state dict, inputs, cotangents, float32 / float64 results."""
    c = CASE
    sd = make_state_dict(NAME, 9, c['seed'])
    imgs = make_inputs(c['B'], c['H'], c['W'], 9, c['seed'])[0]
    dims = tap_dims(c['B'], c['H'], c['W'])
    cot = cotangents(dims, c['cot_seed'] if cot_seed is None else cot_seed, False, zero)
    threads = torch.get_num_threads()
    torch.set_num_threads(REF_THREADS)
    try:
        r32, r64 = grads(sd, imgs, cot, 'float32'), grads(sd, imgs, cot, 'float64')
    finally:
        torch.set_num_threads(threads)
    return dict(sd=sd, imgs=imgs, dims=dims, cot=cot, r32=r32, r64=r64, spread=spreads(r32['grads'], r64['grads']),
                tap_spread=spreads(r32['taps'], r64['taps']))


def sgd_step(p, g, buf, lr, momentum=0.9, weight_decay=5e-4):
    """torch.optim.SGD with coupled weight decay (as ssd_head_ref.sgd_step; float64 numpy)."""
    p, g, buf = (np.asarray(x, np.float64) for x in (p, g, buf))
    buf = momentum * buf + g + weight_decay * p
    return p - lr * buf, buf
