"""CPU checks of the SSD heads' training step: the restatement (tests/ssd_head_ref.py) against torch.nn modules, the learning
rate schedule, and the flat parameter layout of SSD300 (no device work; the C-ABI symbols: tests/test_abi.py)."""
import math

import numpy as np
import pytest
import torch

import ssd_head_ref as R


def _hand_head(seed=0, B=2, H=5, W=4, C=8, n=6):
    g = torch.Generator().manual_seed(seed)
    p = {'0.weight': torch.randn(C, 1, 3, 3, generator=g) * 0.4, '1.weight': torch.rand(C, generator=g) + 0.5,
         '1.bias': torch.randn(C, generator=g) * 0.2, '3.weight': torch.randn(n, C, 1, 1, generator=g) * 0.3,
         '3.bias': torch.randn(n, generator=g) * 0.1}
    tap = torch.randn(B * H * W, C, generator=g)
    do = torch.randn(B * H * W, n, generator=g) * 1e-2
    return p, tap, do, (B, H, W, C, n)


def test_restatement_against_torch_nn_modules():
    p, tap, do, (B, H, W, C, n) = _hand_head()
    seq = torch.nn.Sequential(torch.nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False), torch.nn.BatchNorm2d(C), torch.nn.ReLU(),
                              torch.nn.Conv2d(C, n, 1)).double().train()
    with torch.no_grad():
        for k, v in p.items():
            dict(seq.named_parameters())[k].copy_(v.double())
    x = tap.double().view(B, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    o = seq(x).permute(0, 2, 3, 1).reshape(B * H * W, n)
    (o * do.double()).sum().backward()
    r = R.head_grads(tap, B, H, W, p, do, 'float64')
    assert np.abs(r['out'] - o.detach().numpy()).max() < 1e-12
    for k, v in seq.named_parameters():
        assert np.abs(r[k] - v.grad.numpy()).max() < 1e-12, k
    assert np.abs(r['tap'] - x.grad.permute(0, 2, 3, 1).reshape(B * H * W, C).numpy()).max() < 1e-12
    # the running estimates: momentum 0.1, unbiased variance
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    R.head_forward(tap.double(), B, H, W, {k: v.double() for k, v in p.items()}, torch.float64, running=(rm, rv))
    assert (rm - seq[1].running_mean).abs().max() < 1e-12 and (rv - seq[1].running_var).abs().max() < 1e-12
    # float32 follows float64
    r32 = R.head_grads(tap, B, H, W, p, do, 'float32')
    for k in r:
        assert np.abs(r32[k] - r[k]).max() <= 1e-4 * max(np.abs(r[k]).max(), 1e-6), k


def test_the_half_restatement_is_the_heads_second_half():
    """half_ref (numpy) = the autograd of ReLU(scale*y + shift) -> 1x1 conv with respect to y-side quantities."""
    c = R.half_case('tiny', False)
    assert R.margin_holds(c)
    r = R.half_ref(c, 'float64')
    n = c['n']
    y = torch.from_numpy(c['y'].astype(np.float64))
    u = (torch.from_numpy(c['scale'].astype(np.float64)) * y + torch.from_numpy(c['shift'].astype(np.float64))).requires_grad_(True)
    w = torch.from_numpy(c['w'][:n].astype(np.float64)).requires_grad_(True)
    b = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    o = torch.relu(u) @ w.t() + b
    (o * torch.from_numpy(c['do'][:, :n].astype(np.float64))).sum().backward()
    assert np.abs(r['g'] - u.grad.numpy()).max() < 1e-14
    assert np.abs(r['dW'] - w.grad.numpy()).max() < 1e-14 and np.abs(r['dbias'] - b.grad.numpy()).max() < 1e-14
    assert np.abs(r['stats'][:c['C']] - u.grad.sum(0).numpy()).max() < 1e-14
    assert np.abs(r['stats'][c['C']:] - (u.grad * y).sum(0).numpy()).max() < 1e-14


def test_half_cases_hold_the_mask_margin_and_the_spreads_are_float32_sized():
    for name in R.HALF_SHAPES:
        for bf16 in (False, True):
            c = R.half_case(name, bf16)
            assert R.margin_holds(c), (name, bf16)
            assert (c['do'][:, c['n']:] == 0).all() and (c['w'][c['n']:] == 0).all()
            r32, r64 = R.half_refs(name, bf16)
            assert (r32['mask'] == r64['mask']).all()
    s = R.half_spreads()
    print('float32-against-float64 spreads of the restatement:', s)
    for k, v in s.items():
        assert 0 < v < 1e-4, (k, v)


def test_rounding_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, -3.0 - 2.0 ** -7 - 2.0 ** -30, 1e-3])
    assert (R.round_storage(x, True)[:3] == [1.0, 1.0, 1.0]).all()          # (ties to even; below the half)
    # one rounding: 3 + 2^-7 + 2^-30 lies above the half-way point 3 + 2^-7 of bf16's spacing 2^-6 at 3, float32 drops the 2^-30
    assert R.round_storage(x, True)[3] == -3.0 - 2.0 ** -6
    assert (R.ulp(np.array([1.0, 3.0, 0.75]), True) == [2.0 ** -7, 2.0 ** -6, 2.0 ** -8]).all()
    assert (R.ulp(np.array([1.0]), False) == [2.0 ** -23]).all()


def test_lr_at():
    from torchdet3d.trainer import DetectorHeadTrainer

    class _Det:
        hflat = torch.zeros(8)
    t = DetectorHeadTrainer(_Det())
    assert t.lr_at(0, 0) == pytest.approx(0.05 / 3, rel=1e-15)
    assert t.lr_at(0, 600) == pytest.approx(0.05 * (1 - 0.5 * (2 / 3)), rel=1e-15)
    assert t.lr_at(0, 1200) == 0.05 and t.lr_at(1, 5000) == 0.05
    assert t.lr_at(24, 10 ** 6) == 0.05
    assert t.lr_at(25, 10 ** 6) == pytest.approx(0.005, rel=1e-15)
    assert t.lr_at(30, 10 ** 6) == pytest.approx(0.0005, rel=1e-15)
    assert t.lr_at(35, 10 ** 6) == pytest.approx(0.00005, rel=1e-15)
    for epoch, it in ((0, 0), (0, 1), (0, 600), (0, 1199), (0, 1200), (24, 9999), (25, 3), (29, 10 ** 5), (35, 10 ** 6), (40, 10 ** 6)):
        assert t.lr_at(epoch, it) == pytest.approx(R.lr_at(epoch, it), rel=1e-14), (epoch, it)
    t2 = DetectorHeadTrainer(_Det(), lr=0.1, warmup_iters=4, warmup_ratio=0.5, steps=(2,), gamma=0.5)
    assert [t2.lr_at(0, i) for i in range(5)] == pytest.approx([0.05, 0.0625, 0.075, 0.0875, 0.1], rel=1e-14)
    assert t2.lr_at(2, 100) == pytest.approx(0.05, rel=1e-15)
    assert t.buf.abs().sum() == 0 and t.buf.shape == _Det.hflat.shape


def test_sgd_restatement_against_torch_optim():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(64, generator=g, dtype=torch.float64)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([p], lr=0.05, momentum=0.9, weight_decay=5e-4)
    q, buf = p0.numpy().copy(), np.zeros(64)
    for i in range(3):
        gr = torch.randn(64, generator=g, dtype=torch.float64)
        p.grad = gr.clone()
        opt.step()
        q, buf = R.sgd_step(q, gr.numpy(), buf, 0.05)
        assert np.abs(q - p.detach().numpy()).max() < 1e-14


def test_flat_layout():
    from torchdet3d.models.ssd import flat_head_layout, head_param_shapes
    shapes = head_param_shapes(9)
    lay = flat_head_layout(9)
    learnable = [k for k in shapes if 'running' not in k]
    assert list(lay) == learnable
    end = 0
    for k in learnable:
        off, n = lay[k]
        assert off == end and off % 4 == 0 and n % 4 == 0 and n >= math.prod(shapes[k]), k
        end = off + n
    # a 1x1 conv reserves its rows padded to a multiple of 8: the matrix and bias the kernels read are slices of the buffer
    assert lay['bbox_head.cls_convs.1.3.weight'][1] == 64 * 320 and lay['bbox_head.cls_convs.1.3.bias'][1] == 64
    assert lay['bbox_head.reg_convs.0.3.weight'][1] == 16 * 96


def test_flat_buffers_back_the_parameters():
    """hflat.numel() % 4 == 0 and every learnable head_param_shapes key is a view of it (the running statistics stay outside);
    state_dict / load_state_dict behave as before.  Built on the CPU: the constructor launches nothing."""
    from torchdet3d.models import ssd as S

    class _NoNet:
        def __init__(self, *a, **k):
            pass

        def reset_parameters(self, seed=0):
            pass

        def state_dict(self):
            return {}

        def load_state_dict(self, sd):
            pass
    real, S.Net = S.Net, _NoNet
    try:
        det = S.SSD300(device='cpu', dtype=torch.float32)
        other = S.SSD300(device='cpu', dtype=torch.float32, seed=5)
    finally:
        S.Net = real
    assert det.hflat.numel() % 4 == 0 and det.hflat.dtype == torch.float32 and det.hgrad.shape == det.hflat.shape
    lo, hi = det.hflat.data_ptr(), det.hflat.data_ptr() + det.hflat.numel() * 4
    for k, shp in S.head_param_shapes(9).items():
        assert tuple(det.p[k].shape) == tuple(shp), k
        inside = lo <= det.p[k].data_ptr() and det.p[k].data_ptr() + det.p[k].numel() * 4 <= hi
        assert inside == ('running' not in k), k
        if inside:
            assert det.hg[k].shape == det.p[k].shape and det.hg[k].data_ptr() - det.hgrad.data_ptr() == det.p[k].data_ptr() - lo
    # writing the flat buffer is writing the parameters, and the pads of the padded rows are zero
    o, n = det.hlayout['bbox_head.cls_convs.1.3.weight']
    assert (det.hflat[o + 60 * 320:o + n] == 0).all() and det.hflat[o:o + 60 * 320].abs().min() > 0
    det.hflat[o] = 7.0
    assert det.p['bbox_head.cls_convs.1.3.weight'][0, 0, 0, 0] == 7.0
    assert det.hgrad.abs().sum() == 0
    sd = other.state_dict()
    assert set(sd) == set(S.head_param_shapes(9))
    det.load_state_dict(sd)
    for k in sd:
        assert torch.equal(det.p[k], sd[k]), k
    assert det.hflat.data_ptr() == lo and (det.hflat[o + 60 * 320:o + n] == 0).all()
