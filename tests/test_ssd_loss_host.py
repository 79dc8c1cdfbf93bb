"""CPU checks of the SSD MultiBox loss's definition (tests/ssd_loss_ref.py): hand-worked answers on the 12-anchor set, the
analytic gradients against torch autograd, the float32-against-float64 spreads that bound the kernel's error and the
mining-gap condition of every case tests/test_gpu_ssd_loss.py runs."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ssd_loss_ref as R

SMALL = {c['name']: c for c in R.small_cases()}


def _run(case, dtype=np.float64):
    return R.multibox(case['cls'], case['reg'], R.anchors_of(case), case['gt_boxes'], case['gt_labels'], case['gt_counts'], dtype=dtype)


def test_module_exports_the_loss():
    from torchdet3d.losses import MultiBoxLoss
    from torchdet3d.losses.detection_losses import STDS
    from torchdet3d.models.ssd import SSD300
    assert callable(MultiBoxLoss) and STDS == R.STDS
    assert SSD300.TRAIN_CFG == dict(pos_iou_thr=0.4, neg_iou_thr=0.4, min_pos_iou=0., gt_max_assign_all=False, smoothl1_beta=1.,
                                    neg_pos_ratio=3)


def test_small_anchor_set():
    a = R.small_anchors()
    assert a.shape == (12, 4)
    assert a[0].tolist() == [0, 0, 32, 32] and a[1].tolist() == [8, 8, 24, 24] and a[6].tolist() == [0, 32, 32, 64]
    assert a[8].tolist() == [32, 32, 64, 64]


def test_iou_by_hand():
    a = R.small_anchors()
    v = R.iou_f32([0, 0, 96, 64], a)
    assert (v[0::2] == np.float32(1024) / np.float32(6144)).all() and (v[1::2] == np.float32(256) / np.float32(6144)).all()
    v = R.iou_f32([2, 2, 30, 30], a)
    assert v[0] == np.float32(784) / np.float32(1024) and v[1] == np.float32(256) / np.float32(784) and (v[2:] == 0).all()
    assert (R.iou_f32([1000, 1000, 1050, 1050], a) == 0).all()


@pytest.mark.parametrize('name', list(SMALL))
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_worked_assignment(name, dtype):
    """contained: the tie of the six equal IoUs goes to anchor 0; shared: the later ground truth wins anchor 0; outside:
    anchor 0; invalid: only slot 4 counts; clamp: k = 8 = every negative; tie: the three lowest negatives; empty: nothing."""
    case, r = SMALL[name], _run(SMALL[name], dtype)
    e = case['expect']
    asg = r['assigned'][0]
    assert {int(i): int(asg[i]) for i in range(12) if asg[i] >= 0} == e['positives']
    assert int((asg == -2).sum()) == e['k'] == r['total_mined']
    assert r['num_pos'].tolist() == [len(e['positives'])] and r['total_pos'] == len(e['positives'])
    if 'mined' in e:
        assert np.nonzero(asg == -2)[0].tolist() == e['mined']
    # the mined negatives are the largest ce among the negatives
    neg_ce = r['ce'][0][asg < 0]
    if e['k']:
        assert r['ce'][0][asg == -2].min() >= np.sort(neg_ce)[::-1][e['k'] - 1]


def test_hand_worked_values():
    """contained, worked out in float64: the positive is anchor 0 against the whole image; avg = 1."""
    case, r = SMALL['contained'], _run(SMALL['contained'])
    x, reg = case['cls'][0].astype(np.float64), case['reg'][0].astype(np.float64)
    ce = lambda row, lab: math.log(sum(math.exp(v - row.max()) for v in row)) - (row[lab] - row.max())
    mined = np.nonzero(r['assigned'][0] == -2)[0]
    want = ce(x[0], 3) + sum(ce(x[i], R.NC) for i in mined)
    assert abs(r['loss_cls'] - want) < 1e-12
    s = [float(np.float32(v)) for v in R.STDS]
    t = [(48 - 16) / 32 / s[0], (32 - 16) / 32 / s[1], math.log(96 / 32) / s[2], math.log(64 / 32) / s[3]]
    lb = 0.0
    for q in range(4):
        d = abs(reg[0][q] - t[q])
        lb += 0.5 * d * d if d < 1 else d - 0.5
    assert abs(r['loss_bbox'] - lb) < 1e-12


def test_no_ground_truth_gives_zero():
    r = _run(SMALL['empty'])
    assert r['loss_cls'] == 0 and r['loss_bbox'] == 0 and r['total_pos'] == 0 and r['total_mined'] == 0
    assert (r['assigned'] == -1).all() and (r['dcls'] == 0).all() and (r['dreg'] == 0).all()


@pytest.mark.parametrize('name', ['contained', 'shared', 'clamp', 'tie', 'counts', 'real_fp32'])
def test_analytic_gradients_equal_autograd(name):
    case = next(c for c in R.gpu_cases() if c['name'] == name)
    ref = R.reference(name, 'float64')
    cls = torch.from_numpy(case['cls'].astype(np.float64)).requires_grad_(True)
    reg = torch.from_numpy(case['reg'].astype(np.float64)).requires_grad_(True)
    lc, lb = R.torch_loss(cls, reg, R.anchors_of(case), case['gt_boxes'], ref)
    assert abs(lc.item() - ref['loss_cls']) < 1e-12 * max(1, abs(ref['loss_cls']))
    assert abs(lb.item() - ref['loss_bbox']) < 1e-12 * max(1, abs(ref['loss_bbox']))
    (lc + lb).backward()
    assert np.abs(cls.grad.numpy() - ref['dcls']).max() < 1e-12
    assert np.abs(reg.grad.numpy() - ref['dreg']).max() < 1e-12


def test_spreads_and_mining_gaps_of_the_gpu_cases(capsys):
    """The GPU tolerances are 4 x these spreads; every image of every GPU case keeps the ce at rank k and k + 1 at least 1e-5
    (relative) apart in the float64 restatement, so that an ulp of logf cannot move the selection (the deliberate-tie case
    uses bit-equal rows instead: its gap is exactly 0 and the order is the anchor index)."""
    s = R.spreads()
    with capsys.disabled():
        print('\nfloat32-against-float64 spreads of the restatement over the GPU cases: ' + ', '.join(f'{k} {v:.3e}' for k, v in s.items()))
    assert all(0 < v < 1e-3 for v in s.values())
    for c in R.gpu_cases():
        gaps = R.reference(c['name'], 'float64')['gaps']
        if c['tie']:
            assert gaps == [0.0]
            r32 = R.reference(c['name'], 'float32')
            mined = np.nonzero(r32['assigned'][0] == -2)[0]
            assert len(set(r32['ce'][0][r32['assigned'][0] < 0].view(np.uint32).tolist())) == 1 and mined.tolist() == [1, 2, 3]
        else:
            assert min(gaps) >= 1e-5, (c['name'], gaps)


def test_bad_arguments_are_refused_on_the_host():
    """Argument validation happens in front of the launches: no GPU is needed to see the codes."""
    from torchdet3d import _native as N
    lib = N.lib()
    assert lib.t3d_ssd_multibox_work_bytes(80, 2044) >= 80 * 16 and lib.t3d_ssd_multibox_work_bytes(0, 0) > 0
    assert lib.t3d_ssd_multibox_work_bytes(-1, 4) == N.ERR_ARG
    P, I = ctypes.c_void_p * 1, ctypes.c_int * 1
    d = 4096          # a stand-in device address: every call below returns before anything is launched
    stds = (ctypes.c_float * 4)(*R.STDS)

    def call(**kw):
        a = dict(dtype=N.F32, nlevels=1, cls=P(d), reg=P(d), hw=I(6), na=I(2), cs=I(20), rs=I(8), anchors=d, gb=d, gl=d, gc=d, B=1,
                 G=2, nc=9, pos=0.4, neg=0.4, minpos=0.0, ratio=3, beta=1.0, stds=ctypes.addressof(stds), work=d, wb=16, scalars=d,
                 num_pos=d, assigned=d, dcls=None, dreg=None)
        a.update(kw)
        ad = lambda v: ctypes.addressof(v) if isinstance(v, ctypes.Array) else v
        return lib.t3d_ssd_multibox_loss(a['dtype'], a['nlevels'], ad(a['cls']), ad(a['reg']), ad(a['hw']), ad(a['na']), ad(a['cs']),
                                         ad(a['rs']), a['anchors'], a['gb'], a['gl'], a['gc'], a['B'], a['G'], a['nc'], a['pos'],
                                         a['neg'], a['minpos'], a['ratio'], a['beta'], a['stds'], a['work'], a['wb'], a['scalars'],
                                         a['num_pos'], a['assigned'], ad(a['dcls']), ad(a['dreg']), None)
    assert call(B=0) == 0                                     # nothing to do, nothing launched
    assert call(anchors=None) == N.ERR_ARG and call(scalars=None) == N.ERR_ARG and call(gc=None) == N.ERR_ARG
    assert call(anchors=d + 2) == N.ERR_ARG and call(scalars=d + 4) == N.ERR_ARG and call(work=d + 4) == N.ERR_ARG
    assert call(G=-1) == N.ERR_ARG and call(nlevels=0) == N.ERR_ARG and call(nlevels=3) == N.ERR_ARG
    assert call(wb=8) == N.ERR_ARG and call(dtype=N.F16) == N.ERR_ARG and call(B=-1) == N.ERR_ARG
    assert call(dcls=P(d)) == N.ERR_ARG                       # only one of the two gradient arrays
    assert call(cs=I(19)) == N.ERR_ARG and call(rs=I(7)) == N.ERR_ARG
    assert call(beta=0.0) == N.ERR_ARG and call(ratio=-1) == N.ERR_ARG
    assert call(neg=0.3) == N.ERR_UNSUPPORTED                 # an ignore band is not built
    assert call(G=65) == N.ERR_UNSUPPORTED and call(hw=I(8193)) == N.ERR_UNSUPPORTED      # past the LDS plan: A <= 16384, G <= 64
