"""t3d_ssd_multibox_loss / MultiBoxLoss / SSD300.loss on the device against tests/ssd_loss_ref.py.

Exact: assigned, num_pos, total_pos, total_mined and the zero pattern of the gradients, pad channels included (the IoU and
every decision are exact by construction; the mining-gap condition -- asserted on the CPU by tests/test_ssd_loss_host.py --
keeps an ulp of logf from moving the selection).  Losses and gradients: within 4 x the largest float32-against-float64
difference of the restatement per output kind over all cases of this file (ssd_loss_ref.spreads(), computed on the CPU);
the factor 4 covers the device's expf / logf differing from numpy's by an ulp or so, and nothing else."""
import ctypes

import numpy as np
import pytest
import torch

import ssd_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = {c['name']: c for c in R.gpu_cases()}


def _tol():
    return {k: 4.0 * v for k, v in R.spreads().items()}


def _loss(case):
    from torchdet3d.losses import MultiBoxLoss
    return MultiBoxLoss(torch.from_numpy(R.anchors_of(case)).to(DEV))


def _device_inputs(case):
    lv = case['levels']
    dt = torch.bfloat16 if case['bf16'] else torch.float32
    cls = [torch.from_numpy(x).to(DEV).to(dt) for x in R.to_levels(case['cls'], lv['hws'], lv['nas'], R.NC + 1, case['cls_strides'])]
    reg = [torch.from_numpy(x).to(DEV).to(dt) for x in R.to_levels(case['reg'], lv['hws'], lv['nas'], 4, case['reg_strides'])]
    outs = [(c, r, hw) for c, r, hw in zip(cls, reg, lv['hws'])]
    gt = (torch.from_numpy(case['gt_boxes']).to(DEV), torch.from_numpy(case['gt_labels']).to(DEV), torch.from_numpy(case['gt_counts']).to(DEV))
    return outs, gt


def _run(case, with_grads=True, poison=True):
    outs, gt = _device_inputs(case)
    mb = _loss(case)
    if poison and with_grads:
        # the gradient buffers come from torch.empty: fill the allocator's next blocks with NaN first, so that a channel the
        # kernel fails to write cannot pass as a zero
        junk = [torch.full(o[i].shape, float('nan'), dtype=torch.float32, device=DEV) for o in outs for i in (0, 1)]
        del junk
    r = mb.from_heads(outs, *gt, with_grads=with_grads, nanchors=list(case['levels']['nas']))
    torch.cuda.synchronize()
    return r


def _check(case, r, tol, label=''):
    lv, B = case['levels'], case['cls'].shape[0]
    r32, r64 = R.reference(case['name'], 'float32'), R.reference(case['name'], 'float64')
    assert (r['assigned'].cpu().numpy() == r32['assigned']).all()
    assert (r['num_pos'].cpu().numpy() == r32['num_pos']).all()
    assert r['total_pos'].item() == r32['total_pos'] and r['total_mined'].item() == r32['total_mined']
    errs = dict(loss_cls=abs(r['loss_cls'].item() - r64['loss_cls']), loss_bbox=abs(r['loss_bbox'].item() - r64['loss_bbox']))
    if r['grads'] is not None:
        dcls, pc = R.from_levels([g[0].cpu().numpy() for g in r['grads']], lv['hws'], lv['nas'], R.NC + 1, B)
        dreg, pr = R.from_levels([g[1].cpu().numpy() for g in r['grads']], lv['hws'], lv['nas'], 4, B)
        assert (pc == 0).all() and (pr == 0).all(), 'pad channels of the gradients are written 0'
        unused, notpos = r32['assigned'] == -1, r32['assigned'] < 0
        assert (dcls[unused] == 0).all() and (dreg[notpos] == 0).all()
        assert np.isfinite(dcls).all() and np.isfinite(dreg).all()
        assert (dcls[~unused] != 0).any(-1).all() and ((dreg != 0) == (r64['dreg'] != 0)).all()
        errs['dcls'] = float(np.abs(dcls - r64['dcls']).max())
        errs['dreg'] = float(np.abs(dreg - r64['dreg']).max())
    print(f'{case["name"]}{label}: ' + ', '.join(f'{k} err {v:.3e} (bound {tol[k]:.3e})' for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tol[k], (k, v, tol[k])


@pytest.mark.parametrize('name', list(CASES))
def test_against_the_restatement(name):
    case = CASES[name]
    _check(case, _run(case), _tol())


def test_losses_only():
    """dcls = dreg = NULL: the same scalars and assignment, no gradient written."""
    case = CASES['real_fp32']
    r = _run(case, with_grads=False)
    assert r['grads'] is None
    _check(case, r, _tol(), ' (losses only)')
    g = _run(case)
    for k in ('loss_cls', 'loss_bbox', 'assigned', 'num_pos'):
        assert torch.equal(r[k], g[k])


@pytest.mark.parametrize('name', ['real_bf16', 'tie'])
def test_twice_is_bit_identical(name):
    a, b = _run(CASES[name]), _run(CASES[name])
    for k in ('loss_cls', 'loss_bbox', 'total_pos', 'total_mined', 'assigned', 'num_pos'):
        assert torch.equal(a[k], b[k]), k
    for ga, gb in zip(a['grads'], b['grads']):
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])


def test_empty_batch():
    case = CASES['contained']
    mb = _loss(case)
    outs = [(torch.empty(0, 20, device=DEV), torch.empty(0, 8, device=DEV), 6)]
    gt = (torch.empty(0, 1, 4, device=DEV), torch.empty(0, 1, dtype=torch.int32, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV))
    r = mb.from_heads(outs, *gt, nanchors=[2])
    torch.cuda.synchronize()
    assert r['loss_cls'].item() == 0 and r['loss_bbox'].item() == 0 and r['assigned'].shape == (0, 12)


def test_return_codes():
    from torchdet3d import _native as N
    case = CASES['contained']
    outs, gt = _device_inputs(case)
    mb = _loss(case)
    P, I = ctypes.c_void_p * 1, ctypes.c_int * 1
    host = [P(outs[0][0].data_ptr()), P(outs[0][1].data_ptr()), I(6), I(2), I(20), I(8)]
    work = torch.zeros(2, dtype=torch.float64, device=DEV)
    scal = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    npos = torch.zeros(1, dtype=torch.int32, device=DEV)
    asg = torch.zeros(1, 12, dtype=torch.int32, device=DEV)

    def call(neg=0.4, G=1, wb=16, scalars=scal.data_ptr(), B=1, nl=1):
        return N.lib().t3d_ssd_multibox_loss(N.F32, nl, *[ctypes.addressof(h) for h in host], mb.anchors.data_ptr(), gt[0].data_ptr(),
                                             gt[1].data_ptr(), gt[2].data_ptr(), B, G, 9, 0.4, neg, 0.0, 3, 1.0,
                                             ctypes.addressof(mb._stds), work.data_ptr(), wb, scalars, npos.data_ptr(), asg.data_ptr(),
                                             None, None, N.stream())
    assert call(neg=0.5) == N.ERR_UNSUPPORTED and call(G=65) == N.ERR_UNSUPPORTED
    assert call(wb=8) == N.ERR_ARG and call(scalars=None) == N.ERR_ARG and call(scalars=scal.data_ptr() + 4) == N.ERR_ARG
    assert call(G=-1) == N.ERR_ARG and call(nl=3) == N.ERR_ARG
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert (scal == -7.0).all(), 'a refused call launches nothing'
    assert call() == 0
    torch.cuda.synchronize()
    ref = R.reference('contained', 'float64')
    assert abs(scal[0].item() - ref['loss_cls']) <= _tol()['loss_cls'] and scal[2].item() == 1 and scal[3].item() == 3
    with pytest.raises(RuntimeError):
        from torchdet3d.losses import MultiBoxLoss
        MultiBoxLoss(mb.anchors, neg_iou_thr=0.3).from_heads(outs, *gt, nanchors=[2])


def test_dense_autograd_form():
    """loss(cls_score, bbox_pred, ...) against torch autograd of the float64 restatement; the incoming scalars scale the
    stored gradients (weights 0.5 and 0.25: the bounds scale with them)."""
    case = CASES['dense']
    tol = _tol()
    mb = _loss(case)
    cls = torch.from_numpy(case['cls']).to(DEV).requires_grad_(True)
    reg = torch.from_numpy(case['reg']).to(DEV).requires_grad_(True)
    gt = [torch.from_numpy(case[k]).to(DEV) for k in ('gt_boxes', 'gt_labels', 'gt_counts')]
    lc, lb = mb(cls, reg, *gt)
    (0.5 * lc + 0.25 * lb).backward()
    torch.cuda.synchronize()
    ref = R.reference('dense', 'float64')
    c64 = torch.from_numpy(case['cls'].astype(np.float64)).requires_grad_(True)
    r64 = torch.from_numpy(case['reg'].astype(np.float64)).requires_grad_(True)
    tc, tb = R.torch_loss(c64, r64, R.anchors_of(case), case['gt_boxes'], ref)
    (0.5 * tc + 0.25 * tb).backward()
    errs = dict(loss_cls=abs(lc.item() - tc.item()), loss_bbox=abs(lb.item() - tb.item()),
                dcls=(cls.grad.cpu().double() - c64.grad).abs().max().item() / 0.5,
                dreg=(reg.grad.cpu().double() - r64.grad).abs().max().item() / 0.25)
    print('dense: ' + ', '.join(f'{k} err {v:.3e} (bound {tol[k]:.3e})' for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tol[k], (k, v, tol[k])
    assert ((cls.grad.cpu().numpy() != 0).any(-1) == (ref['assigned'] != -1)).all()


def test_ssd300_loss_is_from_heads_on_its_own_head_outputs():
    from torchdet3d.losses import MultiBoxLoss
    from torchdet3d.models.ssd import SSD300, WIDTHS
    case = CASES['real_bf16']
    det = SSD300(device=DEV, dtype=torch.bfloat16)
    imgs = torch.randint(0, 256, (3, 300, 300, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(DEV)
    gt = [torch.from_numpy(case[k]).to(DEV) for k in ('gt_boxes', 'gt_labels', 'gt_counts')]
    a = det.loss(imgs, *gt, with_grads=True)
    outs = det.head_outputs(imgs)
    b = MultiBoxLoss(det.anchors, **{k: v for k, v in SSD300.TRAIN_CFG.items() if k != 'gt_max_assign_all'}).from_heads(
        outs, *gt, nanchors=[len(w) for w in WIDTHS])
    torch.cuda.synchronize()
    for k in ('loss_cls', 'loss_bbox', 'total_pos', 'total_mined', 'assigned', 'num_pos'):
        assert torch.equal(a[k], b[k]), k
    for ga, gb in zip(a['grads'], b['grads']):
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    assert a['loss_cls'].item() > 0 and a['loss_bbox'].item() > 0 and a['total_pos'].item() == R.reference('real_bf16', 'float32')['total_pos']
    assert det.loss(imgs, *gt)['grads'] is None


def test_a_recorded_plan_replays_the_call():
    """The call recorded into a plan and replayed over new logits in the same tensors gives what a fresh call gives."""
    from torchdet3d import _native as N
    case = CASES['real_bf16']
    outs, gt = _device_inputs(case)
    mb = _loss(case)
    nas = list(case['levels']['nas'])
    rec = N.PlanRecorder()
    N.recorder = rec
    try:
        r = mb.from_heads(outs, *gt, nanchors=nas)
        rec.end_segment()
    finally:
        N.recorder = None
    try:
        torch.cuda.synchronize()
        first = r['loss_cls'].item()
        for c, _, _ in outs:
            c.mul_(0.5)                      # (exact in bf16; the NaN pads stay NaN)
        slots = (ctypes.c_ulonglong * N.NSLOTS)()
        assert N.lib().t3d_plan_run(rec.plan, 0, slots, N.NSLOTS, None, 0) >= 0
        torch.cuda.synchronize()
        fresh = mb.from_heads(outs, *gt, nanchors=nas)
        torch.cuda.synchronize()
        assert r['loss_cls'].item() != first
        for k in ('loss_cls', 'loss_bbox', 'total_pos', 'total_mined', 'assigned', 'num_pos'):
            assert torch.equal(r[k], fresh[k]), k
        for ga, gb in zip(r['grads'], fresh['grads']):
            assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    finally:
        rec.close()
