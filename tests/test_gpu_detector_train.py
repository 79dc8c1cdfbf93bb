"""Net.forward_taps_train / Net.backward_taps, SSD300.train_backward and DetectorTrainer on the device, against
tests/ssd_backbone_ref.py (the tapped backbone in training mode) and tests/ssd_head_ref.py (the heads).

Bounds.  Backbone gradients and train-mode taps, fp32 storage: per tensor the largest error against the float64 restatement,
relative to max(that tensor's largest float64 magnitude, 1e-3 x the largest gradient of all), is at most 4 x the
float32-against-float64 spread of the restatement on the same case (the margin of tests/test_gpu_ssd_head_train.py; the case and
its conditioning: tests/test_detector_train_host.py).  Running statistics: the tolerances of tests/test_gpu_golden.py (mean atol
1e-5, variance rtol 1e-4).  Head gradients of `train_backward`: 4 x the spread of ssd_head_ref's autograd on the device's own
train-mode taps and the device's own dcls / dreg.  One `DetectorTrainer.train_step`: the restatement's SGD step on the device's
own gradients, per element 4 * 2^-24 * (|p'| + lr * |buf|).  Everything else is bit equality.
The tables the tests print are in DESIGN.md section 7 (b2).

Recorded on an MI355X:
  backward_taps, fp32 storage: taps 6.78e-06 (spread 6.12e-06, bound 2.45e-05) and 2.85e-05 (2.38e-05, 9.51e-05); all 153 gradient
  tensors inside their bounds, median error 1.78e-05 against a median spread of 1.70e-05, closest features.15.conv.8.bias 2.00e-06
  of 3.34e-06; each tap alone: closest 4.34e-06 of 8.01e-06 (middle tap alone), 2.71e-06 of 4.53e-06 (deepest alone);
  y-free join forced, bf16: worst tensor 3.7e-02 from the default route (relative L2), median 1.1e-02;
  train_backward, fp32 storage, B = 2 with counts 1 / 8: head gradients inside their bounds, closest the 1x1 weight of the
  320-channel box head 9.2e-08 of 3.0e-07; bf16 storage against the fp32-storage run (recorded, not bounded): backbone 1.6e-03 ..
  1.4 of each tensor's floored scale (median 0.85), heads 2.0e-02 .. 0.86;
  one train_step: worst ratio to the bound 0.43 (heads), 0.61 (backbone); eight steps on one batch: loss 22.52 -> 6.35, eval-path
  loss 22.79 -> 20.85;
  the stride-2 depthwise shapes pass on the parent commit as well.
"""
import ctypes

import numpy as np
import pytest
import torch

import ssd_backbone_ref as R
import ssd_head_ref as RH

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAPS = R.TAPS


def _N():
    from torchdet3d import _native as N
    return N


def _net(dtype, sd=None):
    from torchdet3d.models.engine import Net
    net = Net(R.NAME, 9, DEV, dtype)
    net.load_state_dict(R.case()['sd'] if sd is None else sd)
    return net


def _tapped_pass(net, c):
    """One forward_taps_train + backward_taps on case `c` -> (taps {k: float64 numpy rows}, gflat clone)."""
    taps = net.forward_taps_train(c['imgs'].to(DEV), TAPS)
    for k in TAPS:
        assert taps[k][1:] == c['dims'][k] and taps[k][0].dtype == net.dtype
    got = {k: taps[k][0].double().cpu().numpy() for k in TAPS}
    net.backward_taps({k: c['cot'][k].to(DEV).to(net.dtype).contiguous() for k in TAPS})
    torch.cuda.synchronize()
    assert net.saved is None
    return got, net.gflat.clone()


_RUNS = {}


def _fp32_run(zero=()):
    """The case's pass on a fresh fp32-storage net, computed once per cotangent pattern and shared."""
    if zero not in _RUNS:
        net = _net(torch.float32)
        before = net.state_dict()
        taps, gflat = _tapped_pass(net, R.case(zero))
        _RUNS[zero] = dict(net=net, before=before, after=net.state_dict(), taps=taps, gflat=gflat,
                           grads={k: net.g[k].double().cpu().numpy() for k in net.g})
    return _RUNS[zero]


def _check_grads(run, c, label):
    """Every stem / features.* gradient within 4 x its float32 spread of the float64 restatement; prints the table."""
    rows, bad = [], []
    for k, ref in c['r64']['grads'].items():
        spread, scale = c['spread'][k]
        err = float(np.abs(run['grads'][k].reshape(ref.shape) - ref).max()) / scale
        rows.append((k, spread, 4 * spread, err))
        if not err <= 4 * spread:
            bad.append((k, err, 4 * spread))
    print(f'{label}: tensor, float32 spread, bound, error')
    for k, s, b, e in rows:
        print(f'  {k}: {s:.3e} {b:.3e} {e:.3e}')
    worst = max(rows, key=lambda r: r[3] / max(r[2], 1e-300))
    print(f'{label}: closest to its bound: {worst[0]} error {worst[3]:.3e} of {worst[2]:.3e}; '
          f'median error {np.median([r[3] for r in rows]):.3e}, median spread {np.median([r[1] for r in rows]):.3e}')
    assert not bad, bad[:10]


def _assert_zero_outside_features(net, gflat):
    used = torch.zeros_like(gflat, dtype=torch.bool)
    for k in net.g:
        if k.startswith('features.'):
            o, n = net.offsets[k]
            used[o:o + n] = True
    assert (gflat[~used] == 0).all(), 'a gradient element outside the stem and features.* is not exactly 0'
    assert used[:net.offsets['conv.0.weight'][0]].any() and not used[net.offsets['conv.0.weight'][0]:].any()


# ---- 1 -------------------------------------------------------------------------------------------------------------------
def test_backward_taps_against_float64_autograd():
    c, run = R.case(), _fp32_run()
    for k in TAPS:
        spread, scale = c['tap_spread'][k]
        err = float(np.abs(run['taps'][k] - c['r64']['taps'][k]).max()) / scale
        print(f'tap features.{k}: spread {spread:.3e} bound {4 * spread:.3e} error {err:.3e}')
        assert err <= 4 * spread, (k, err, 4 * spread)
    _check_grads(run, c, 'backward_taps')
    _assert_zero_outside_features(run['net'], run['gflat'])
    after, before, ref = run['after'], run['before'], c['r64']['buffers']
    seen = 0
    for k, v in after.items():
        if k in run['net'].p:
            assert torch.equal(v, before[k]), f'{k}: a pass without an optimizer changed a parameter'
        elif not k.startswith('features.'):
            assert torch.equal(v, before[k]), f'{k}: a buffer behind the deepest tap changed'
        elif k.endswith('running_mean'):
            np.testing.assert_allclose(v.cpu().numpy(), ref[k], atol=1e-5, rtol=0, err_msg=k)
            assert not torch.equal(v, before[k]), k
            seen += 1
        elif k.endswith('running_var'):
            np.testing.assert_allclose(v.cpu().numpy(), ref[k], rtol=1e-4, atol=1e-6, err_msg=k)
        else:
            assert int(v) == int(before[k]) + 1 == int(ref[k]), k
    assert seen == 1 + 2 + 3 * 16            # the stem's, features.1's two and three per expanded block


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero', [(17,), (13,)], ids=['middle_tap_alone', 'deepest_tap_alone'])
def test_each_tap_alone(zero):
    c, run = R.case(zero), _fp32_run(zero)
    if zero == (17,):
        for k, v in run['grads'].items():
            if k.startswith('features.') and int(k.split('.')[1]) >= 14:
                assert (v == 0).all(), f'{k}: no gradient reaches features.14 .. 17 through the middle tap'
    _check_grads(run, c, f'cotangent at features.{zero[0]} zero')
    _assert_zero_outside_features(run['net'], run['gflat'])


def test_middle_tap_joins_in_the_y_free_expansion_backward_too():
    """At the config's batch (80 x 19 x 19 rows, 96 -> 576) the expansion backward of features.14 takes the y-free route
    (`Net._yfree_ok`: bf16, M * N >= 8 M elements), which receives the tap gradient through its own `residual` argument; two
    images never reach that threshold, so the route is forced here for the three 96 -> 576 expansions (features.12 .. 14;
    the first two carry a skip connection's gradient there, as in the regression step).  With the deepest tap's cotangent zero
    everything below features.14 is fed through the join alone: a route that dropped the residual would give exact zeros, a
    relative distance of 1.  Bound: 0.25 in the relative L2 sense per tensor (floored scale) against the default bf16 route --
    the route rounds its concatenated weights to bf16 once more (1.5e-2 of the largest entry at the layer itself,
    tests/test_gpu_pwconv.py), and a ReLU6 kink that flips under that perturbation moves a tensor by up to 2e-1
    (tests/test_detector_train_host.py); anything structural is of order 1."""
    N = _N()
    dims = R.tap_dims(2, 300, 300)          # the detector's planes: 2 x 19 x 19 = 722 rows at the join
    c = dict(imgs=torch.randn(2, 3, 300, 300, generator=torch.Generator().manual_seed(7)), dims=dims,
             cot=R.cotangents(dims, 1, True, zero=(17,)))
    base = _net(torch.bfloat16)
    _, g0 = _tapped_pass(base, c)
    net = _net(torch.bfloat16)
    net._yfree_ok = lambda x, M, K, Nn: (K, Nn) == (96, 576)
    _tapped_pass(net, c)                # (buffers and packs exist: the recorded pass below is the launches alone)
    rec = N.PlanRecorder()
    N.recorder = rec
    try:
        _, g1 = _tapped_pass(net, c)
    finally:
        N.recorder = None
        names = [x[0] for x in rec.calls]
        rec.close()
    yfree = [n for n in names if 'yfree' in n and ('dgrad' in n or 'bwd_yfree_w' in n)]
    print('y-free data-gradient launches of the forced pass:', yfree)
    assert len(yfree) == 3 and not any('yfree' in x for x in _names_of_default_pass(base, c))
    gmax = float(g0.abs().max())
    # the projection BatchNorm shifts of features.1 .. 10 feed nothing but 1x1 convs in front of mean-subtracting BatchNorms
    # (the skip chains end at features.11, which has none): their true gradient is 0 (float64 autograd: 1e-16 of the largest
    # gradient), what either bf16 run holds there is its own rounding, and two roundings are not compared
    noise = {f'features.{i}.conv.{5 if i == 1 else 8}.bias' for i in range(1, 11)}
    rows = []
    for k, (o, n) in net.offsets.items():
        if k.startswith('features.') and int(k.split('.')[1]) <= 13:
            a, b = g1[o:o + n].double(), g0[o:o + n].double()
            assert (a != 0).any(), k
            if k not in noise:
                rows.append((float((a - b).norm() / max(float(b.norm()), R.SCALE_FLOOR * gmax * n ** 0.5)), k))
    print(f'forced y-free route against the default bf16 route, relative L2 per tensor: worst {max(rows)}, '
          f'median {np.median([r[0] for r in rows]):.3e}; above 0.05: {[r for r in sorted(rows, reverse=True) if r[0] > 0.05]}')
    assert max(rows)[0] <= 0.25, max(rows)
    for k, (o, n) in net.offsets.items():
        if k.startswith('features.') and int(k.split('.')[1]) >= 14:
            assert (g1[o:o + n] == 0).all(), k


def _names_of_default_pass(net, c):
    N = _N()
    rec = N.PlanRecorder()
    N.recorder = rec
    try:
        _tapped_pass(net, c)
    finally:
        N.recorder = None
        names = [x[0] for x in rec.calls]
        rec.close()
    return names


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_a_tap_in_front_of_a_skip_connection_is_refused():
    run = _fp32_run()
    net = _net(torch.float32)
    c = R.case()
    before = net.state_dict()
    with pytest.raises(NotImplementedError, match='features.13'):
        net.forward_taps_train(c['imgs'].to(DEV), (12, 17))
    assert net.saved is None and all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    _, gflat = _tapped_pass(net, c)
    assert torch.equal(gflat.view(torch.int32), run['gflat'].view(torch.int32))


def test_gradient_hooks_cover_the_whole_flat_buffer(monkeypatch):
    """The all-reduce hooks of a data-parallel wrapper fire over all of `gflat`, from its end towards 0, and with a hook
    attached the gradients are the ones without (the bucket size is lowered so that this small net has several buckets)."""
    import torchdet3d.models.engine as E
    monkeypatch.setattr(E, 'HOOK_MIN', 1 << 18)
    net = _net(torch.float32)
    los = []
    net.grad_hook = los.append
    _, gflat = _tapped_pass(net, R.case())
    n = net.offsets['conv.0.weight'][0]
    assert len(los) >= 3 and los[-1] == 0 and all(a > b for a, b in zip(los, los[1:])) and los[0] < n
    assert all(lo in {o for o, _ in net.offsets.values()} for lo in los)
    assert torch.equal(gflat.view(torch.int32), _fp32_run()['gflat'].view(torch.int32))


# ---- 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_reproducible_and_nothing_leaks_into_the_other_passes(dtype):
    N = _N()
    c = R.case()
    a, b = _net(dtype), _net(dtype)
    _, g1 = _tapped_pass(a, c)
    _, g2 = _tapped_pass(b, c)
    _, g3 = _tapped_pass(b, c)          # (a second pass on the same net: other running estimates, same batch statistics)
    assert torch.isfinite(g1).all() and (g1 != 0).any()
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g3.view(torch.int32))
    if dtype == torch.float32:
        assert torch.equal(g1.view(torch.int32), _fp32_run()['gflat'].view(torch.int32))
    # inference taps after a tapped training pass: those of a fresh net with the same state, launch for launch
    imgs = c['imgs'].to(DEV)
    sd = a.state_dict()
    fresh = _net(dtype, sd)
    fresh.forward_taps(imgs, TAPS)      # (packs the weights: launches of a first pass only)
    torch.cuda.synchronize()
    n0 = N.launch_count()
    tf = {k: v[0].clone() for k, v in fresh.forward_taps(imgs, TAPS).items()}
    n1 = N.launch_count()
    ta = {k: v[0].clone() for k, v in a.forward_taps(imgs, TAPS).items()}
    n2 = N.launch_count()
    torch.cuda.synchronize()
    assert n2 - n1 == n1 - n0 > 0
    for k in TAPS:
        assert torch.equal(ta[k].view(torch.uint8), tf[k].view(torch.uint8)), k
    # a regression step after a tapped training pass: that of a fresh net with the same state, bit for bit
    _, gt_kp, cats = __import__('oracle.weights', fromlist=['make_inputs']).make_inputs(R.CASE['B'], R.CASE['H'], R.CASE['W'], 9)
    g = torch.Generator().manual_seed(5)
    dkp, dlg = torch.randn(R.CASE['B'], 18, generator=g).to(DEV), torch.randn(R.CASE['B'], 9, generator=g).to(DEV)
    ones = torch.ones(R.CASE['B'], 1280, device=DEV)
    fresh2 = _net(dtype, sd)
    outs = []
    for net in (a, fresh2):
        kp, lg = net.forward(imgs, cats.to(DEV), train=True, dropout_mask=ones)
        net.backward(dkp, dlg)
        torch.cuda.synchronize()
        outs.append((kp.clone(), lg.clone(), net.gflat.clone(), net.state_dict()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2].view(torch.int32), outs[1][2].view(torch.int32)) and (outs[0][2] != 0).any()
    assert all(torch.equal(v, outs[1][3][k]) for k, v in outs[0][3].items())
    with pytest.raises(AssertionError):
        a.backward_taps({})             # the regression pass's saved state is not a tapped pass's (and is consumed)


# ---- 5 -------------------------------------------------------------------------------------------------------------------
_TB = {}


def _train_backward_fp32():
    """train_backward on a fresh fp32-storage detector (B = 2, ground-truth counts 1 and 8) + the same three pieces called
    one by one on a second detector, whose train-mode taps feed ssd_head_ref; computed once."""
    if _TB:
        return _TB
    from test_gpu_ssd_head_train import _batch, _det
    from torchdet3d.models.ssd import BRANCHES
    batch = _batch(2, (1, 8))
    det = _det(torch.float32)
    sd0 = {k: v.clone() for k, v in det.state_dict().items()}
    r = det.train_backward(*batch)
    torch.cuda.synchronize()
    det2 = _det(torch.float32)
    taps = det2.backbone.forward_taps_train(batch[0], TAPS)
    tap_rows = {k: taps[k][0].float().cpu() for k in TAPS}
    r2 = det2._heads_fwd_bwd(taps, 2, *batch[1:], True)
    det2.backbone.backward_taps(dict(zip(TAPS, r2['dtaps'])))
    torch.cuda.synchronize()
    ref32, ref64 = {}, {}
    threads = torch.get_num_threads()
    torch.set_num_threads(R.REF_THREADS)        # (the float32 spreads depend on the summation order: ssd_backbone_ref.py)
    try:
        for l, k in enumerate(TAPS):
            _, B, H, W, C = taps[k]
            acc32, acc64 = 0, 0
            for bi, br in enumerate(BRANCHES):
                p = f'bbox_head.{br}.{l}'
                prm = {kk: sd0[f'{p}.{kk}'].cpu() for kk in RH.HEAD_KEYS}
                n = prm['3.bias'].shape[0]
                do = r['grads'][l][bi].cpu()[:, :n]
                g32 = RH.head_grads(tap_rows[k], B, H, W, prm, do, 'float32')
                g64 = RH.head_grads(tap_rows[k], B, H, W, prm, do, 'float64')
                for kk in RH.HEAD_KEYS:
                    ref32[f'{p}.{kk}'], ref64[f'{p}.{kk}'] = g32[kk], g64[kk]
                acc32, acc64 = acc32 + g32['tap'], acc64 + g64['tap']
            ref32[f'tap{l}'], ref64[f'tap{l}'] = acc32, acc64
    finally:
        torch.set_num_threads(threads)
    got = {k: det.hg[k].double().cpu().numpy() for k in det.hg}
    for l in range(len(TAPS)):
        got[f'tap{l}'] = r['dtaps'][l].double().cpu().numpy()
    _TB.update(det=det, det2=det2, batch=batch, r=r, sd0=sd0, got=got, ref32=ref32, ref64=ref64)
    return _TB


def test_train_backward_is_its_three_pieces():
    t = _train_backward_fp32()
    det, det2 = t['det'], t['det2']
    g1, g2 = det.backbone.gflat, det2.backbone.gflat
    assert torch.isfinite(g1).all() and (g1 != 0).any()
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert torch.equal(det.hgrad.view(torch.int32), det2.hgrad.view(torch.int32))
    _assert_zero_outside_features(det.backbone, g1)
    for k, v in det.backbone.g.items():
        if k.startswith('features.'):
            assert (v != 0).any(), f'{k}: no gradient arrived'
    rows = []
    for k in sorted(t['got']):
        ref64, ref32 = t['ref64'][k], t['ref32'][k]
        scale = np.abs(ref64).max()
        assert scale > 0 and np.isfinite(t['got'][k]).all(), k
        rows.append((k, np.abs(ref32.reshape(ref64.shape) - ref64).max() / scale,
                     np.abs(t['got'][k].reshape(ref64.shape) - ref64).max() / scale))
    for k, spread, err in rows:
        print(f'{k}: spread {spread:.3e} bound {4 * spread:.3e} err {err:.3e}')
    for k, spread, err in rows:
        assert err <= 4 * spread, (k, err, 4 * spread)
    # the backbone's BatchNorms ran in training mode: every features.* estimate moved, nothing behind the taps did
    bb = det.backbone.state_dict()
    for k, v in bb.items():
        old = t['sd0']['backbone.' + k] if ('backbone.' + k) in t['sd0'] else None
        if old is None:
            continue
        if k.startswith('features.') and ('running' in k or k.endswith('tracked')):
            assert not torch.equal(v, old), f'{k} did not move'
        else:
            assert torch.equal(v, old), f'{k} changed'


def test_train_backward_without_a_ground_truth_and_in_bf16():
    from test_gpu_ssd_head_train import _batch, _det
    for dtype in (torch.float32, torch.bfloat16):
        det = _det(dtype)
        rm0 = det.backbone.buffers['features.17.conv.8.running_mean'].clone()
        hm0 = det.p['bbox_head.cls_convs.1.1.running_mean'].clone()
        r = det.train_backward(*_batch(1, (0,)))
        torch.cuda.synchronize()
        assert r['total_pos'].item() == 0
        assert (det.hgrad == 0).all() and (det.backbone.gflat == 0).all(), 'without a ground truth every gradient is exactly 0'
        assert not torch.equal(det.backbone.buffers['features.17.conv.8.running_mean'], rm0)
        assert not torch.equal(det.p['bbox_head.cls_convs.1.1.running_mean'], hm0)
    t = _train_backward_fp32()
    det = _det(torch.bfloat16)
    r = det.train_backward(*t['batch'])
    torch.cuda.synchronize()
    assert torch.isfinite(det.hgrad).all() and torch.isfinite(det.backbone.gflat).all() and (det.backbone.gflat != 0).any()
    assert all(torch.isfinite(x.float()).all() for x in r['dtaps'])
    f32 = t['det'].backbone
    rel = {}
    gmax = max(float(v.abs().max()) for k, v in f32.g.items() if k.startswith('features.'))
    for k, v in det.backbone.g.items():
        if k.startswith('features.'):
            b = f32.g[k].double()
            rel[k] = float((v.double() - b).abs().max() / max(float(b.abs().max()), R.SCALE_FLOOR * gmax))
    hrel = {k: float((det.hg[k].double() - t['det'].hg[k].double()).abs().max() / t['det'].hg[k].double().abs().max().clamp(min=1e-30))
            for k in det.hg}
    print('bf16 storage against fp32 storage, relative to the largest magnitude (recorded, not bounded): backbone '
          f'{min(rel.values()):.2e} .. {max(rel.values()):.2e} (median {np.median(list(rel.values())):.2e}), heads '
          f'{min(hrel.values()):.2e} .. {max(hrel.values()):.2e}')
    assert all(np.isfinite(x) for x in list(rel.values()) + list(hrel.values()))


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_one_train_step_is_the_restatements_sgd_step():
    from test_gpu_ssd_head_train import _det
    from torchdet3d.trainer import DetectorTrainer
    t = _train_backward_fp32()
    det = _det(torch.float32)
    bb = det.backbone
    n = bb.offsets['conv.0.weight'][0]
    h0, f0 = det.hflat.double().cpu().numpy(), bb.flat.clone()
    tr = DetectorTrainer(det, warmup_iters=4)
    assert tr.nbackbone == n
    lc, lb, tot = tr.train_step(*t['batch'])
    torch.cuda.synchronize()
    assert lc.item() == t['r']['loss_cls'].item() and lb.item() == t['r']['loss_bbox'].item() and tot.item() == lc.item() + lb.item()
    lr = RH.lr_at(0, 0, warmup_iters=4)
    assert lr == tr.lr_at(0, 0)
    # the device's own gradients (the step leaves them in place; they are train_backward's, bit for bit)
    assert torch.equal(det.hgrad.view(torch.int32), t['det'].hgrad.view(torch.int32))
    assert torch.equal(bb.gflat.view(torch.int32), t['det'].backbone.gflat.view(torch.int32))
    for label, p0, g, got, buf_dev in (('heads', h0, det.hgrad, det.hflat, tr.buf),
                                       ('backbone', f0[:n].double().cpu().numpy(), bb.gflat[:n], bb.flat[:n], tr.bbuf)):
        want, buf = R.sgd_step(p0, g.double().cpu().numpy(), np.zeros_like(p0), lr)
        bound = 4 * 2.0 ** -24 * (np.abs(want) + lr * np.abs(buf)) + 1e-30
        err = np.abs(got.double().cpu().numpy() - want)
        print(f'train_step, {label}: largest error {err.max():.3e}, largest bound {bound.max():.3e}, worst ratio {(err / bound).max():.3f}')
        assert (err <= bound).all(), label
        assert np.abs(buf_dev.double().cpu().numpy() - buf).max() <= 4 * 2.0 ** -24 * np.abs(buf).max()
    assert torch.equal(bb.flat[n:].view(torch.int32), f0[n:].view(torch.int32)), 'a parameter the detector does not use changed'
    assert (bb.flat[n:] != 0).any()
    for k, (o, m) in bb.offsets.items():
        if k.startswith('features.'):
            assert (bb.flat[o:o + m] != f0[o:o + m]).any(), f'{k} did not move'


# ---- 7 -------------------------------------------------------------------------------------------------------------------
def _train8():
    from test_gpu_ssd_head_train import _batch, _det
    from torchdet3d.trainer import DetectorTrainer
    det = _det(torch.bfloat16)
    batch = _batch(2, (2, 2), seed=1)
    before = det.loss(*batch)
    before = (before['loss_cls'] + before['loss_bbox']).item()
    tr = DetectorTrainer(det, warmup_iters=4)
    losses = [tr.train_step(*batch)[2] for _ in range(8)]
    torch.cuda.synchronize()
    after = det.loss(*batch)
    after = (after['loss_cls'] + after['loss_bbox']).item()
    return det, [x.item() for x in losses], before, after


def test_eight_train_steps_lower_the_loss_reproducibly():
    det_a, la, before, after = _train8()
    det_b, lb, _, _ = _train8()
    print('losses over eight steps:', ' '.join(f'{x:.4f}' for x in la), f'| eval-path loss {before:.4f} -> {after:.4f}')
    assert all(np.isfinite(la)) and la[7] < la[0]
    assert torch.equal(det_a.hflat.view(torch.int32), det_b.hflat.view(torch.int32)) and la == lb
    assert torch.equal(det_a.backbone.flat.view(torch.int32), det_b.backbone.flat.view(torch.int32))
    assert np.isfinite(after) and after != before
    assert not det_a.backbone.nonfinite()


# ---- 8 -------------------------------------------------------------------------------------------------------------------
def test_a_recorded_train_backward_replays():
    from test_gpu_ssd_head_train import _batch, _det
    N = _N()
    det = _det(torch.bfloat16)
    bb = det.backbone
    batch = _batch(2, (1, 3), seed=2)
    det.train_backward(*batch)              # (buffers exist, the packs are made)
    torch.cuda.synchronize()
    rec = N.PlanRecorder()
    N.recorder = rec
    try:
        r = det.train_backward(*batch)
        rec.end_segment()
    finally:
        N.recorder = None
    try:
        torch.cuda.synchronize()
        assert rec.broken is None
        rec_h, rec_g = det.hgrad.clone(), bb.gflat.clone()
        for v in det.hg.values():
            v.fill_(float('nan'))
        bb.gflat.fill_(float('nan'))
        for t in r['dtaps']:
            t.fill_(float('nan'))
        slots = (ctypes.c_ulonglong * N.NSLOTS)()
        assert N.lib().t3d_plan_run(rec.plan, 0, slots, N.NSLOTS, None, 0) >= 0
        torch.cuda.synchronize()
        rep_h, rep_g, loss_replayed = det.hgrad.clone(), bb.gflat.clone(), r['loss_cls'].item()
        fresh = det.train_backward(*batch)
        torch.cuda.synchronize()
        assert torch.isfinite(rep_h).all() and torch.isfinite(rep_g).all() and (rep_g != 0).any()
        for a, b in ((rep_h, det.hgrad), (rep_h, rec_h), (rep_g, bb.gflat), (rep_g, rec_g)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert loss_replayed == fresh['loss_cls'].item()
    finally:
        rec.close()


# ---- 9 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,H', [(96, 150), (144, 75), (192, 38), (576, 19)])
def test_detector_stride2_depthwise_shapes(C, H, monkeypatch):
    """The stride-2 depthwise layers of the backbone at 300 x 300 (planes 150 -> 75 -> 38 -> 19 -> 10, two of the inputs odd),
    one image: forward with batch sums, backward with dx, dW and the producer's sums -- the checks and bounds of
    tests/test_gpu_production_shapes.py at these shapes (its batch size replaced).  They pass on the parent commit too: no
    kernel needed a change for the detector's planes."""
    import test_gpu_production_shapes as P
    monkeypatch.setattr(P, 'B', 1)
    P.test_dw3_forward_production_shape(C, H, 2)
    P.test_dw3_backward_production_shape(C, H, 2)
