"""Restatement of the SSD heads' training step on the CPU (numpy / torch): the definition tests/test_ssd_head_host.py and
tests/test_gpu_ssd_head_train.py hold csrc/ssd_head_bwd.hip, SSD300.head_backward and DetectorHeadTrainer to.

A head (mmdet's SSDHead with depthwise heads, configs/detection/mnv2_ssd_300_2_heads.py:15-37 of the reference) is
    depthwise 3x3 conv, pad 1, no bias -> BatchNorm2d in TRAINING mode (batch statistics, biased variance, eps 1e-5; running
    estimates moved with momentum 0.1 and the unbiased variance) -> ReLU -> 1x1 conv with bias
on NHWC rows [B*H*W, C].  Its gradients come from torch autograd in the requested dtype.  The 1x1 half alone (what
t3d_ssd_head_bwd computes) is restated in numpy in float32 and float64.  The implementing mmdetection fork is external to
the reference, so parity with the reference's detector stays unpinned: the published mmdet / torch.nn definitions and this file
are the definition.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
MASK_MARGIN = 1e-3          # every |scale*y + shift| >= MASK_MARGIN * |scale|: the fp64 sign of the ReLU argument is the fp32 sign

# name -> (M, C, n, ns): the four real heads at B = 3 (19x19 and 10x10 maps), a shape below any tile, a single row, and
# several workgroups with a ragged last one
HALF_SHAPES = {
    'cls0': (1083, 96, 40, 40), 'reg0': (1083, 96, 16, 16), 'cls1': (300, 320, 60, 64), 'reg1': (300, 320, 24, 24),
    'tiny': (37, 8, 4, 8), 'one_row': (1, 96, 40, 40), 'ragged': (4099, 96, 16, 16),
}
REAL_HEADS = ('cls0', 'reg0', 'cls1', 'reg1')


def stored(x, bf16):
    """x (float32 numpy) as the storage dtype holds it, widened back to float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy() if bf16 else x


@functools.lru_cache(maxsize=None)
def half_case(name, bf16):
    """Seeded inputs of the 1x1 half: do [M, ns] fp32 (pad columns 0, by the loss's contract), y [M, C] and w [ns, C] as
    STORED (pad rows 0), scale / shift [C] fp32 -- drawn so that the mask margin holds (offending y redrawn)."""
    M, C, n, ns = HALF_SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 2 + int(bf16))
    do = np.zeros((M, ns), np.float32)
    do[:, :n] = rng.standard_normal((M, n)).astype(np.float32) * rng.choice([0., 1e-3, 1e-2], (M, 1), p=[.25, .5, .25]).astype(np.float32)
    w = np.zeros((ns, C), np.float32)
    w[:n] = rng.standard_normal((n, C)).astype(np.float32) * np.float32(np.sqrt(2.0 / C))
    scale = (rng.uniform(0.5, 2.0, C) * rng.choice([-1., 1.], C, p=[.1, .9])).astype(np.float32)
    shift = rng.uniform(-1.0, 1.0, C).astype(np.float32)
    y = stored(rng.standard_normal((M, C)).astype(np.float32), bf16)
    for _ in range(100):
        bad = np.abs(scale.astype(np.float64) * y + shift) < 2 * MASK_MARGIN * np.abs(scale)
        if not bad.any():
            break
        y[bad] = stored(rng.standard_normal(int(bad.sum())).astype(np.float32), bf16)
    out = dict(name=name, bf16=bf16, M=M, C=C, n=n, ns=ns, do=do, y=y, w=stored(w, bf16), scale=scale, shift=shift)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def margin_holds(c):
    u = c['scale'].astype(np.float64) * c['y'] + c['shift']
    return bool((np.abs(u) >= MASK_MARGIN * np.abs(c['scale'])).all())


def half_ref(c, dtype):
    """The 1x1 half in `dtype` (float32: every operation in float32): g [M, C] unrounded, mask, stats [2C] = sum(g), sum(g*y),
    dW [n, C], dbias [n]."""
    dt = np.dtype(dtype)
    n = c['n']
    do, y, w = c['do'][:, :n].astype(dt), c['y'].astype(dt), c['w'][:n].astype(dt)
    u = c['scale'].astype(dt) * y + c['shift'].astype(dt)
    mask = u > 0
    g = (do @ w) * mask
    a = np.where(mask, u, dt.type(0))
    return dict(g=g, mask=mask, stats=np.concatenate([g.sum(0, dtype=dt), (g * y).sum(0, dtype=dt)]), dW=do.T @ a, dbias=do.sum(0, dtype=dt))


@functools.lru_cache(maxsize=None)
def half_refs(name, bf16):
    c = half_case(name, bf16)
    return half_ref(c, 'float32'), half_ref(c, 'float64')


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


HALF_OUTPUTS = ('dW', 'dbias', 'stats_g', 'stats_gy')


def split_outputs(r, C):
    return dict(dW=r['dW'], dbias=r['dbias'], stats_g=r['stats'][:C], stats_gy=r['stats'][C:])


@functools.lru_cache(maxsize=None)
def half_spreads():
    """Per output the largest float32-against-float64 difference of the restatement, relative to the output's largest
    magnitude, over every case of this file in both storage dtypes."""
    out = dict.fromkeys(HALF_OUTPUTS, 0.0)
    for name in HALF_SHAPES:
        for bf16 in (False, True):
            r32, r64 = half_refs(name, bf16)
            C = HALF_SHAPES[name][1]
            a, b = split_outputs(r32, C), split_outputs(r64, C)
            for k in HALF_OUTPUTS:
                out[k] = max(out[k], _rel(a[k], b[k]))
    return out


def round_storage(g64, bf16):
    """fp64 -> the storage dtype, one rounding (bf16: round to nearest even on the fp64 value), as float64."""
    g64 = np.asarray(g64, np.float64)
    if not bf16:
        return g64.astype(np.float32).astype(np.float64)
    f = g64.astype(np.float32)
    # round-to-odd to float32 first, so that the bf16 rounding is the single rounding of the fp64 value
    bits = f.view(np.uint32).copy()
    inexact = f.astype(np.float64) != g64
    low = np.abs(f.astype(np.float64)) < np.abs(g64)
    even = (bits & 1) == 0
    bits = np.where(inexact & even, np.where(low, bits + 1, bits - 1), bits).astype(np.uint32)
    return torch.from_numpy(bits.view(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def ulp(x, bf16):
    """Spacing of the storage dtype at |x| (x: float64 values representable in it)."""
    x = np.abs(np.asarray(x, np.float64))
    if not bf16:
        return np.spacing(x.astype(np.float32)).astype(np.float64)
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 7)


# ---- a whole head, autograd -----------------------------------------------------------------------------------------------
HEAD_KEYS = ('0.weight', '1.weight', '1.bias', '3.weight', '3.bias')


def head_forward(tap, B, H, W, p, dtype, running=None):
    """tap [B*H*W, C] rows (NHWC) -> head output rows [B*H*W, n]; p: {'0.weight' [C,1,3,3], '1.weight', '1.bias' [C], '3.weight'
    [n,C,1,1], '3.bias' [n]} torch tensors of `dtype`.  `running` = (mean, var) float64 tensors, updated in place."""
    C = tap.shape[1]
    x = tap.view(B, H, W, C).permute(0, 3, 1, 2)
    y = F.conv2d(x, p['0.weight'], None, 1, 1, 1, C)
    mean = y.mean((0, 2, 3))
    var = y.var((0, 2, 3), unbiased=False)
    if running is not None:
        cnt = B * H * W
        with torch.no_grad():
            running[0].mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean.double())
            running[1].mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var.double() * (cnt / (cnt - 1) if cnt > 1 else 1.0))
    z = (y - mean[None, :, None, None]) / torch.sqrt(var + BN_EPS)[None, :, None, None] * p['1.weight'][None, :, None, None] \
        + p['1.bias'][None, :, None, None]
    o = F.conv2d(F.relu(z), p['3.weight'], p['3.bias'])
    return o.permute(0, 2, 3, 1).reshape(B * H * W, -1)


def head_grads(tap, B, H, W, p, do, dtype):
    """Gradients of sum(out * do) -- `do` [B*H*W, n] is the loss's gradient at the head output -- with respect to the five
    parameters and the tap, in `dtype`: {key: numpy float64}, 'tap' included; plus the output under 'out'."""
    dt = torch.float64 if dtype == 'float64' else torch.float32
    q = {k: torch.as_tensor(v).to(dt).clone().requires_grad_(True) for k, v in p.items()}
    t = torch.as_tensor(tap).to(dt).clone().requires_grad_(True)
    o = head_forward(t, B, H, W, q, dt)
    (o * torch.as_tensor(do).to(dt)).sum().backward()
    out = {k: v.grad.double().numpy() for k, v in q.items()}
    out['tap'] = t.grad.double().numpy()
    out['out'] = o.detach().double().numpy()
    return out


# ---- optimizer ------------------------------------------------------------------------------------------------------------
def sgd_step(p, g, buf, lr, momentum=0.9, weight_decay=5e-4):
    """torch.optim.SGD, coupled weight decay, dampening 0, no Nesterov: -> (p, buf) after the step (float64 numpy)."""
    p, g, buf = (np.asarray(x, np.float64) for x in (p, g, buf))
    d = g + weight_decay * p
    buf = momentum * buf + d
    return p - lr * buf, buf


def lr_at(epoch, it, lr=0.05, warmup_iters=1200, warmup_ratio=1 / 3, steps=(25, 30, 35), gamma=0.1):
    """mmcv's LrUpdaterHook, policy 'step' with linear warm-up by iteration (config :147-153)."""
    regular = lr * gamma ** sum(1 for s in steps if epoch >= s)
    if it < warmup_iters:
        k = (1 - it / warmup_iters) * (1 - warmup_ratio)
        return regular * (1 - k)
    return regular
