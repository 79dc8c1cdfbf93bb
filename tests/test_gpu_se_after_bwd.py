"""The gate-after-activation backward of a squeeze-excite block as ONE launch (t3d_se_after_bwd, csrc/se.hip) and as the
three-launch sequence it replaces (t3d_se_after_sums -> t3d_se_bwd_data -> t3d_se_after_apply), both against fp64 torch
autograd of the same expression

    u = scale*y + shift,  a = act(u),  m = mean_hw a,  h = relu(W1 m + b1),  q = W2 h + b2,  s = h_sigmoid(q),  v = s*a

with dv the gradient at v: du = dL/du, g = dL/dm / HW, dq = dL/dq, dp = dL/d(W1 m + b1), BatchNorm sums sum(du), sum(du*y).

Tolerances: the form of tests/test_gpu_loss_head.py::test_se_gate_fwd_bwd -- rtol 1e-4, atol 2e-5 * max(1, |ref|max); the
sums atol 1e-3 * sqrt(B) [* sqrt(HW) for sum(du*y)].  Two things follow from the number formats, not from the kernels:
  * du is STORED in the activation dtype.  In bf16 storage a stored value is the fp32 result rounded to 8 significant bits
    (half an ulp = 2^-9 relative); an fp32 error of 1e-4 relative may also move it across a rounding boundary, so the bf16
    bound on du is one ulp, rtol 2^-8, with the same atol.  The sums are taken over the STORED du (that is the contract: the
    BatchNorm backward must describe the tensor the next kernel reads), so their reference is the sum of the reference du
    rounded to the storage dtype.
  * act' is discontinuous (ReLU at 0, h-swish at +-3).  The inputs are drawn on a grid (y in 1/64 steps, scale in quarter
    steps, shift in 1/32 steps) on which u is exact in fp32 and fp64 alike, so no sample sits within rounding of a kink on
    one side only; at the kinks themselves the kernels follow PyTorch's conventions (common.h: act_grad)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, R, HW, act): the eight gated blocks of mobilenetv3_large_21k at 224^2 (six distinct shapes) ...
PRODUCTION = [(72, 24, 784, 'relu'), (120, 32, 784, 'relu'), (480, 120, 196, 'hswish'), (672, 168, 196, 'hswish'),
              (672, 168, 49, 'hswish'), (960, 240, 49, 'hswish')]
# ... + B = 1, B = 5, HW = 1 and a channel count that is not a multiple of 64 (72, 120 and 200 are not)
CASES = [(256, *p) for p in PRODUCTION] + [(1, 120, 32, 784, 'relu'), (5, 672, 168, 49, 'hswish'), (7, 960, 240, 1, 'hswish'),
                                           (3, 200, 56, 100, 'hswish')]


def _problem(B, C, R, HW, act, dtype):
    g = torch.Generator().manual_seed(B * 1000 + C + HW)
    y = (torch.randint(-200, 201, (B, HW, C), generator=g).float() / 64).to(dtype)          # exact in bf16 too
    dv = (torch.randn(B, HW, C, generator=g) * 0.1).to(dtype)
    scale = torch.tensor([0.5, 0.75, 1.0, 1.5, 2.0])[torch.randint(0, 5, (C,), generator=g)]
    shift = torch.randint(-32, 33, (C,), generator=g).float() / 32
    w1 = torch.randn(R, C, generator=g) / C ** .5
    b1 = torch.randn(R, generator=g) * .1
    w2 = torch.randn(C, R, generator=g) / R ** .5
    b2 = torch.randn(C, generator=g) * .5
    return [t.cuda() for t in (y, dv, scale, shift, w1, b1, w2, b2)]


def _reference(y, dv, scale, shift, w1, b1, w2, b2, act, dtype):
    """fp64 torch autograd (on the device: 34 M elements per tensor at the largest shape)."""
    d = lambda t: t.double()
    u = (d(scale) * d(y) + d(shift)).requires_grad_(True)
    a = F.relu(u) if act == 'relu' else u * (F.relu6(u + 3) / 6)
    m = a.mean(1)
    m.retain_grad()
    pre = F.linear(m, d(w1), d(b1))
    pre.retain_grad()
    h = F.relu(pre)
    q = F.linear(h, d(w2), d(b2))
    q.retain_grad()
    s = F.relu6(q + 3) / 6
    v = s[:, None, :] * a
    (v * d(dv)).sum().backward()
    HW = y.shape[1]
    du_stored = u.grad.to(dtype).double()
    ref = dict(du=u.grad, g=m.grad / HW, dq=q.grad, dp=pre.grad, st0=du_stored.sum((0, 1)), st1=(du_stored * d(y)).sum((0, 1)))
    fwd = dict(pooled=m.detach().float().contiguous(), h=h.detach().float().contiguous(), q=q.detach().float().contiguous(),
               s=s.detach().float().contiguous())
    return {k: v.detach() for k, v in ref.items()}, fwd


def _run(path, N, dt, y, dv, pro, w1, w2, fwd, B, HW, C, R, nrep):
    """-> du, g, dq, dp, stats [2C] (replicas summed in index order)."""
    dev = y.device
    du = torch.empty_like(y)
    g, dq, dp = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev), torch.empty(B, R, device=dev)
    stats = torch.zeros(nrep, 2 * C, device=dev, dtype=torch.float64)
    st = N.stream()
    N.call('t3d_set_reduction_replicas', nrep, 2 * C)
    try:
        if path == 'fused':
            N.call('t3d_se_after_bwd', dt, N.ptr(dv), N.ptr(y), pro, N.ptr(w1), N.ptr(w2), N.ptr(fwd['h']), N.ptr(fwd['q']),
                   N.ptr(fwd['s']), N.ptr(g), N.ptr(dq), N.ptr(dp), N.ptr(du), N.ptr(stats), B, HW, C, R, st)
        else:
            ps = torch.empty(B, C, 2, device=dev)
            ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
            N.call('t3d_se_after_sums', dt, N.ptr(dv), N.ptr(y), pro, N.ptr(ps), B, HW, C, st)
            N.call('t3d_se_bwd_data', N.ptr(ps), N.ptr(fwd['pooled']), N.ptr(zeros), N.ptr(ones), N.ptr(w1), N.ptr(w2),
                   N.ptr(fwd['h']), N.ptr(fwd['q']), N.ptr(fwd['s']), N.ptr(g), N.ptr(dq), N.ptr(dp), None, B, C, R, HW, st)
            N.call('t3d_se_after_apply', dt, N.ptr(dv), N.ptr(y), pro, N.ptr(fwd['s']), N.ptr(g), N.ptr(du), N.ptr(stats),
                   B, HW, C, st)
        torch.cuda.synchronize()
    finally:
        N.call('t3d_set_reduction_replicas', 1, 0)
    total = stats[0].clone()
    for r in range(1, nrep):
        total += stats[r]
    return du, g, dq, dp, total


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('B,C,R,HW,act', CASES)
def test_se_after_bwd_one_launch_and_sequence_against_fp64_autograd(B, C, R, HW, act, dtype):
    from torchdet3d import _native as N
    dt = N.BF16 if dtype == torch.bfloat16 else N.F32
    y, dv, scale, shift, w1, b1, w2, b2 = _problem(B, C, R, HW, act, dtype)
    ref, fwd = _reference(y, dv, scale, shift, w1, b1, w2, b2, act, dtype)
    pro = N.prologue(scale, shift, None, act, False)
    du_rtol = 2.0 ** -8 if dtype == torch.bfloat16 else 1e-4

    def close(name, got, want, rtol=1e-4):
        want = want.cpu().numpy()
        err = np.abs(got.double().cpu().numpy() - want)
        print(f'  {name}: max abs err {err.max():.3e} (|ref|max {np.abs(want).max():.3e})')
        np.testing.assert_allclose(got.double().cpu().numpy(), want, rtol=rtol, atol=2e-5 * max(1., np.abs(want).max()),
                                   err_msg=name)

    outs = {}
    for path, nrep in (('fused', 4), ('sequence', 1)):
        print(f'[{path} B={B} C={C} R={R} HW={HW} {act} {dtype}]')
        du, g, dq, dp, st = outs[path] = _run(path, N, dt, y.view(B * HW, C), dv.view(B * HW, C), pro, w1, w2, fwd, B, HW, C, R, nrep)
        close('du', du.view(B, HW, C), ref['du'], du_rtol)
        close('g', g, ref['g'])
        close('dq', dq, ref['dq'])
        close('dp', dp, ref['dp'])
        for i, k, tol in ((0, 'st0', 1e-3 * B ** .5), (1, 'st1', 1e-3 * B ** .5 * HW ** .5)):
            got, want = st[i * C:(i + 1) * C].cpu().numpy(), ref[k].cpu().numpy()
            print(f'  {k}: max abs err {np.abs(got - want).max():.3e} (atol {tol:.3e})')
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=tol, err_msg=k)
    # the one-launch kernel twice: identical bits
    again = _run('fused', N, dt, y.view(B * HW, C), dv.view(B * HW, C), pro, w1, w2, fwd, B, HW, C, R, 4)
    for name, a, b in zip(('du', 'g', 'dq', 'dp', 'stats'), outs['fused'], again):
        assert torch.equal(a, b), name


def test_se_after_bwd_rejects_what_it_does_not_take():
    from torchdet3d import _native as N
    z = torch.zeros(64, device='cuda')
    p = N.ptr(z)
    args = lambda C, R: (N.F32, p, p, None, p, p, p, p, p, p, p, p, p, None, 1, 1, C, R, N.stream())
    lib = N.lib()
    assert lib.t3d_se_after_bwd(*args(12, 4)) == -1          # C % 8
    assert lib.t3d_se_after_bwd(*args(2048, 8)) == -3        # wider than the kernel's LDS plan
    assert lib.t3d_se_after_bwd(N.F16, *args(8, 8)[1:]) == -1
