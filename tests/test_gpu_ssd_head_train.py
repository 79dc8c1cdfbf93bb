"""t3d_ssd_head_bwd, SSD300.head_backward and DetectorHeadTrainer on the device against tests/ssd_head_ref.py.

Bounds.  The kernel's dW, dbias and both halves of stats: the largest error against the float64 restatement, relative to that
output's largest magnitude, is at most 4 x the float32-against-float64 spread of the restatement over the file's cases
(ssd_head_ref.half_spreads(), computed on the CPU) -- the rule of tests/test_gpu_ssd_loss.py.  g: the float64 result rounded to
the storage dtype, to within one unit in the last place of that dtype; the ReLU mask exact (the inputs keep
|scale*y + shift| >= 1e-3 |scale|, asserted on the CPU before the launch).  head_backward in fp32 storage: per tensor 4 x the
spread between the restatement's float32 and float64 autograd on the same taps.

Recorded on an MI355X (relative to each output's largest magnitude; the largest over the cases):
  kernel, 7 shapes x 2 storage dtypes: dW 1.13e-07 (spread 4.75e-07, bound 1.90e-06), dbias 4.82e-08 (2.00e-06, 8.01e-06),
  stats_g 2.10e-15 (1.36e-06, 5.44e-06), stats_gy 2.57e-15 (1.28e-06, 5.13e-06); g: 0 ulp in fp32 and in bf16 storage;
  head_backward, fp32 storage, B = 3 with counts 0 / 1 / 8: every tensor inside its bound; closest: the depthwise weight of
  the 320-channel class head 1.54e-06 (spread 6.06e-07, bound 2.42e-06), the 1x1 weight of the 320-channel box head 3.34e-07
  (2.48e-07, 9.90e-07); dtaps 1.12e-07 / 1.03e-07 (bounds 5.19e-07 / 7.02e-07);
  head_backward, bf16 storage against the fp32-storage run (recorded, not bounded: the taps themselves differ by the
  backbone's bf16 rounding, and with them the mined negatives): parameter gradients 4.7e-04 .. 2.4e-01, dtaps 3.6e-01 / 5.2e-01;
  one train_step: largest parameter error 0.25 of its bound; eight steps on one batch: loss 21.67 -> 6.95.
"""
import ctypes

import numpy as np
import pytest
import torch

import ssd_head_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _N():
    from torchdet3d import _native as N
    return N


def _arrs(vals, kind):
    return (kind * len(vals))(*vals)


def _call_half(cases, bf16, sentinel=float('nan'), dtype_code=None, override=None):
    """One t3d_ssd_head_bwd call over `cases` (dicts of ssd_head_ref.half_case) -> (rc, per case dict of device outputs)."""
    N = _N()
    dt = torch.bfloat16 if bf16 else torch.float32
    nh = len(cases)
    dev, outs = [], []
    for c in cases:
        M, C, n, ns = c['M'], c['C'], c['n'], c['ns']
        dev.append(dict(do=torch.from_numpy(c['do'].copy()).to(DEV), y=torch.from_numpy(c['y'].copy()).to(DEV).to(dt),
                        w=torch.from_numpy(c['w'].copy()).to(DEV).to(dt), scale=torch.from_numpy(c['scale'].copy()).to(DEV),
                        shift=torch.from_numpy(c['shift'].copy()).to(DEV)))
        outs.append(dict(g=torch.full((M, C), sentinel, device=DEV).to(dt), stats=torch.zeros(2 * C, dtype=torch.float64, device=DEV),
                         dW=torch.full((n, C), sentinel, device=DEV), dbias=torch.full((n,), sentinel, device=DEV)))
    geo = {k: [c[k] for c in cases] for k in ('M', 'C', 'n', 'ns')}
    if override:
        geo.update(override)
    I = {k: _arrs(v, ctypes.c_int) for k, v in geo.items()}
    nb = N.lib().t3d_ssd_head_bwd_work_bytes(nh, *[ctypes.addressof(I[k]) for k in ('M', 'C', 'n')])
    work = torch.empty(max(nb, 16) // 8 + 2, dtype=torch.float64, device=DEV)
    P = {k: _arrs([d[k].data_ptr() for d in dev], ctypes.c_void_p) for k in ('do', 'y', 'scale', 'shift', 'w')}
    Q = {k: _arrs([o[k].data_ptr() for o in outs], ctypes.c_void_p) for k in ('g', 'stats', 'dW', 'dbias')}
    a = ctypes.addressof
    rc = N.lib().t3d_ssd_head_bwd(N.dtype_code(outs[0]['g']) if dtype_code is None else dtype_code, nh, a(P['do']), a(P['y']),
                                  a(P['scale']), a(P['shift']), a(P['w']), a(I['M']), a(I['C']), a(I['n']), a(I['ns']), N.ACT['relu'],
                                  a(Q['g']), a(Q['stats']), a(Q['dW']), a(Q['dbias']), N.ptr(work), max(nb, 0), N.stream())
    torch.cuda.synchronize()
    return rc, outs


def _check_half(c, o, errs, ulps):
    bf16 = c['bf16']
    assert R.margin_holds(c)                       # so the fp64 sign of the ReLU argument is the fp32 sign
    r64 = R.half_refs(c['name'], bf16)[1]
    g = o['g'].double().cpu().numpy()
    assert np.isfinite(g).all() and ((g != 0) <= r64['mask']).all(), 'the mask is the forward\'s ReLU bit'
    want = R.round_storage(r64['g'], bf16)
    assert ((g == 0) >= ~r64['mask']).all()
    d = np.abs(g - want) / R.ulp(want, bf16)
    ulps[bf16] = max(ulps.get(bf16, 0.0), float(d.max()))
    got = R.split_outputs(dict(dW=o['dW'].cpu().numpy(), dbias=o['dbias'].cpu().numpy(), stats=o['stats'].cpu().numpy()), c['C'])
    ref = R.split_outputs(r64, c['C'])
    for k in R.HALF_OUTPUTS:
        assert np.isfinite(got[k]).all(), k
        errs[k] = max(errs.get(k, 0.0), R._rel(got[k], ref[k]))


def _assert_half(errs, ulps, label):
    tol = {k: 4.0 * v for k, v in R.half_spreads().items()}
    print(f'{label}: ' + ', '.join(f'{k} err {errs[k]:.3e} (spread {tol[k] / 4:.3e}, bound {tol[k]:.3e})' for k in R.HALF_OUTPUTS)
          + '; g ulps ' + ', '.join(f'{"bf16" if b else "fp32"} {v:.3f}' for b, v in ulps.items()))
    for k in R.HALF_OUTPUTS:
        assert errs[k] <= tol[k], (k, errs[k], tol[k])
    for b, v in ulps.items():
        assert v <= 1.0, ('g is more than one unit in the last place away', b, v)


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_kernel_four_real_heads_in_one_call(bf16):
    cases = [R.half_case(n, bf16) for n in R.REAL_HEADS]
    rc, outs = _call_half(cases, bf16)
    assert rc == 0
    errs, ulps = {}, {}
    for c, o in zip(cases, outs):
        _check_half(c, o, errs, ulps)
    _assert_half(errs, ulps, f'four heads {"bf16" if bf16 else "fp32"}')


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', ['tiny', 'one_row', 'ragged'])
def test_kernel_single_head(name, bf16):
    c = R.half_case(name, bf16)
    rc, outs = _call_half([c], bf16)
    assert rc == 0
    errs, ulps = {}, {}
    _check_half(c, outs[0], errs, ulps)
    _assert_half(errs, ulps, f'{name} {"bf16" if bf16 else "fp32"}')


@pytest.mark.parametrize('names', [('ragged',), R.REAL_HEADS], ids=['ragged', 'four_heads'])
def test_kernel_twice_is_bit_identical(names):
    for bf16 in (False, True):
        cases = [R.half_case(n, bf16) for n in names]
        rc1, a = _call_half(cases, bf16)
        rc2, b = _call_half(cases, bf16, sentinel=float('inf'))
        assert rc1 == 0 and rc2 == 0
        for x, y in zip(a, b):
            for k in x:
                assert torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)), (names, bf16, k)


def test_kernel_return_codes():
    N = _N()
    base = R.half_case('tiny', False)

    def untouched(outs):
        return all(bool((o[k] == 5.0).all()) for o in outs for k in ('g', 'dW', 'dbias')) and all(bool((o['stats'] == 0).all()) for o in outs)
    for override, dtype_code, want in (({'C': [12]}, None, N.ERR_UNSUPPORTED), ({'ns': [72]}, None, N.ERR_UNSUPPORTED),
                                       ({'n': [9]}, None, N.ERR_ARG), (None, N.F16, N.ERR_UNSUPPORTED),
                                       ({'C': [1032]}, None, N.ERR_UNSUPPORTED), ({'n': [0]}, None, N.ERR_ARG)):
        rc, outs = _call_half([base], False, sentinel=5.0, dtype_code=dtype_code, override=override)
        assert rc == want, (override, dtype_code, rc)
        assert untouched(outs), (override, dtype_code)
    # nothing to do: no launch, outputs untouched
    before = N.launch_count()
    rc, outs = _call_half([base], False, sentinel=5.0, override={'M': [0]})
    assert rc == 0 and untouched(outs) and N.launch_count() == before
    assert N.lib().t3d_ssd_head_bwd(N.F32, 0, *([None] * 9), N.ACT['relu'], *([None] * 5), 0, N.stream()) == 0
    assert N.launch_count() == before
    # a valid call is two launches
    rc, outs = _call_half([base], False, sentinel=5.0)
    assert rc == 0 and N.launch_count() == before + 2 and not untouched(outs)


# ---- SSD300.head_backward ---------------------------------------------------------------------------------------------------
def _batch(B, counts, G=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (B, 300, 300, 3), dtype=torch.uint8, generator=g)
    xy = torch.rand(B, G, 2, generator=g) * 180 + 10
    wh = torch.rand(B, G, 2, generator=g) * 90 + 30
    boxes = torch.cat([xy, xy + wh], -1).float()
    labels = torch.randint(0, 9, (B, G), generator=g, dtype=torch.int32)
    return imgs.to(DEV), boxes.to(DEV), labels.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)


_SCALES = []


def _tap_scales():
    """1 / std of each tap of the seeded backbone (fp32 storage, one probe batch), computed once: the seeded backbone's taps are
    tiny, and a head BatchNorm whose input variance drowns in eps would test little of its backward."""
    if not _SCALES:
        from torchdet3d.models.ssd import SSD300, TAPS
        det = SSD300(device=DEV, dtype=torch.float32)
        taps = det.backbone.forward_taps(_batch(2, (0, 0), seed=9)[0], TAPS)
        _SCALES.extend(1.0 / float(taps[k][0].float().std()) for k in TAPS)
    return _SCALES


def _det(dtype, seed=0):
    from torchdet3d.models.ssd import SSD300
    scales = _tap_scales()
    det = SSD300(device=DEV, dtype=dtype, seed=seed)
    for k, v in det.p.items():
        if k.endswith('.0.weight'):        # the depthwise output -- the BatchNorm's input -- gets a variance of order 1
            v.mul_(scales[int(k.split('.')[2])])
    # BatchNorm parameters away from their initial 1 / 0, biases away from 0: every gradient path carries a signal
    g = torch.Generator().manual_seed(100 + seed)
    for k, v in det.p.items():
        if k.endswith('.1.weight'):
            v.copy_((torch.rand(v.shape, generator=g) + 0.5).to(DEV))
        elif k.endswith('.1.bias') or k.endswith('.3.bias'):
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(DEV))
    det.params_changed()
    return det


_HB = {}


def _head_backward_fp32(counts):
    """One fp32-storage head_backward with tap gradients + the restatement's float32 / float64 autograd on the device's own
    taps and the device's own dcls / dreg; computed once per case and shared."""
    key = tuple(counts)
    if key in _HB:
        return _HB[key]
    from torchdet3d.models.ssd import BRANCHES, TAPS
    B = len(counts)
    det = _det(torch.float32)
    batch = _batch(B, counts)
    sd0 = {k: v.clone() for k, v in det.state_dict().items()}
    bb0 = {k: v.clone() for k, v in det.backbone.state_dict().items()}
    r = det.head_backward(*batch, tap_grads=True)
    torch.cuda.synchronize()
    taps = det.backbone.forward_taps(batch[0], TAPS)
    torch.cuda.synchronize()
    ref32, ref64, running = {}, {}, {}
    for l, k in enumerate(TAPS):
        t, _, H, W, C = taps[k]
        tap = t.float().cpu()
        acc32, acc64 = 0, 0
        for bi, br in enumerate(BRANCHES):
            p = f'bbox_head.{br}.{l}'
            prm = {kk: sd0[f'{p}.{kk}'].cpu() for kk in R.HEAD_KEYS}
            n = prm['3.bias'].shape[0]
            do = r['grads'][l][bi].cpu()[:, :n]
            g32, g64 = R.head_grads(tap, B, H, W, prm, do, 'float32'), R.head_grads(tap, B, H, W, prm, do, 'float64')
            for kk in R.HEAD_KEYS:
                ref32[f'{p}.{kk}'], ref64[f'{p}.{kk}'] = g32[kk], g64[kk]
            acc32, acc64 = acc32 + g32['tap'], acc64 + g64['tap']
            rm, rv = sd0[f'{p}.1.running_mean'].double().cpu(), sd0[f'{p}.1.running_var'].double().cpu()
            R.head_forward(tap.double(), B, H, W, {kk: v.double() for kk, v in prm.items()}, torch.float64, running=(rm, rv))
            running[f'{p}.1.running_mean'], running[f'{p}.1.running_var'] = rm.numpy(), rv.numpy()
        ref32[f'tap{l}'], ref64[f'tap{l}'] = acc32, acc64
    got = {k: det.hg[k].double().cpu().numpy() for k in det.hg}
    for l in range(len(TAPS)):
        got[f'tap{l}'] = r['dtaps'][l].double().cpu().numpy()
    out = dict(det=det, batch=batch, r=r, got=got, ref32=ref32, ref64=ref64, running=running, sd0=sd0, bb0=bb0,
               hflat0=None)
    _HB[key] = out
    return out


@pytest.mark.parametrize('counts', [(0, 1, 8), (0,)], ids=['b3', 'b1_empty'])
def test_head_backward_against_autograd(counts):
    h = _head_backward_fp32(counts)
    got, ref32, ref64 = h['got'], h['ref32'], h['ref64']
    assert set(got) == set(ref64)
    if sum(counts) == 0:
        for k, v in got.items():
            assert (v == 0).all(), f'{k}: without a ground truth every gradient is exactly 0'
        assert h['r']['total_pos'].item() == 0
    else:
        rows = []
        for k in sorted(got):
            scale = np.abs(ref64[k]).max()
            assert scale > 0 and np.isfinite(got[k]).all(), k
            spread = np.abs(ref32[k].reshape(ref64[k].shape) - ref64[k]).max() / scale
            err = np.abs(got[k].reshape(ref64[k].shape) - ref64[k]).max() / scale
            rows.append((k, spread, err))
        for k, spread, err in rows:
            print(f'{k}: spread {spread:.3e} bound {4 * spread:.3e} err {err:.3e}')
        for k, spread, err in rows:
            assert err <= 4 * spread, (k, err, 4 * spread)
    # the flat gradient buffer's pads stay zero
    det = h['det']
    used = torch.zeros_like(det.hgrad, dtype=torch.bool)
    for k in det.hg:
        o = det.hlayout[k][0]
        used[o:o + det.hg[k].numel()] = True
    assert (det.hgrad[~used] == 0).all()


@pytest.mark.parametrize('counts', [(0, 1, 8), (0,)], ids=['b3', 'b1_empty'])
def test_running_statistics_move_and_the_backbone_does_not(counts):
    h = _head_backward_fp32(counts)
    det = h['det']
    for k, want in h['running'].items():
        got = det.p[k].double().cpu().numpy()
        before = h['sd0'][k].double().cpu().numpy()
        assert np.abs(got - before).max() > 0, f'{k} did not move'
        # float32 arithmetic on fp64 sums: a few float32 roundings of values of the statistics' own size
        assert np.abs(got - want).max() <= 8 * 2.0 ** -24 * max(np.abs(want).max(), 1.0), k
    bb = det.backbone.state_dict()
    assert set(bb) == set(h['bb0'])
    for k, v in h['bb0'].items():
        assert torch.equal(bb[k], v), f'backbone.{k} changed'


def test_head_backward_bf16_against_fp32_storage():
    """bf16 storage: the finite / zero pattern, and the relative error against the fp32-storage run -- recorded (module
    docstring), not bounded: the bf16 taps already differ from the fp32 ones by the backbone's rounding, and the mined negatives
    with them."""
    h = _head_backward_fp32((0, 1, 8))
    det = _det(torch.bfloat16)
    r = det.head_backward(*h['batch'], tap_grads=True)
    torch.cuda.synchronize()
    assert det.hflat.dtype == torch.float32 and r['dtaps'][0].dtype == torch.bfloat16
    assert torch.isfinite(det.hgrad).all() and all(torch.isfinite(t.float()).all() for t in r['dtaps'])
    rel = {}
    for k in det.hg:
        a, b = det.hg[k].double().cpu().numpy(), h['got'][k]
        assert (a != 0).any(), k
        rel[k] = float(np.abs(a - b).max() / np.abs(b).max())
    for l, t in enumerate(r['dtaps']):
        a, b = t.double().cpu().numpy(), h['got'][f'tap{l}']
        rel[f'tap{l}'] = float(np.abs(a - b).max() / np.abs(b).max())
    print('bf16 storage against fp32 storage, relative to the largest magnitude: ' + ', '.join(f'{k} {v:.2e}' for k, v in rel.items()))
    assert all(np.isfinite(v) for v in rel.values())
    # without a ground truth: exactly zero in bf16 storage too
    det1 = _det(torch.bfloat16)
    det1.head_backward(*_batch(1, (0,)), tap_grads=False)
    torch.cuda.synchronize()
    assert (det1.hgrad == 0).all()


def _grad_tol(h):
    """Absolute tolerance of every hgrad element: 4 x the float32 spread of its tensor (the head_backward bound)."""
    det = h['det']
    tol = torch.zeros_like(det.hgrad, dtype=torch.float64)
    ref = torch.zeros_like(tol)
    for k in det.hg:
        o, n = det.hlayout[k][0], det.hg[k].numel()
        tol[o:o + n] = 4 * float(np.abs(h['ref32'][k].reshape(h['ref64'][k].shape) - h['ref64'][k]).max())
        ref[o:o + n] = torch.from_numpy(h['ref64'][k].reshape(-1)).to(DEV)
    return ref, tol


def test_one_train_step_is_the_restatements_sgd_step():
    from torchdet3d.trainer import DetectorHeadTrainer
    h = _head_backward_fp32((0, 1, 8))
    det = _det(torch.float32)
    p0 = det.hflat.double().cpu().numpy()
    tr = DetectorHeadTrainer(det, warmup_iters=4)
    lc, lb, tot = tr.train_step(*h['batch'])
    torch.cuda.synchronize()
    assert lc.item() == h['r']['loss_cls'].item() and lb.item() == h['r']['loss_bbox'].item() and tot.item() == lc.item() + lb.item()
    ref, tol = _grad_tol(h)
    lr = R.lr_at(0, 0, warmup_iters=4)
    assert lr == tr.lr_at(0, 0)
    want, buf = R.sgd_step(p0, ref.cpu().numpy(), np.zeros_like(p0), lr)
    got = det.hflat.double().cpu().numpy()
    # the gradient tolerance times lr, plus the float32 roundings of the step's own arithmetic (on the parameter and on the update)
    bound = lr * tol.cpu().numpy() + 4 * 2.0 ** -24 * (np.abs(want) + lr * np.abs(buf)) + 1e-30
    err = np.abs(got - want)
    print(f'train_step: largest parameter error {err.max():.3e}, largest bound {bound.max():.3e}, worst ratio {(err / bound).max():.3f}')
    assert (err <= bound).all()
    assert np.abs(got - p0).max() > 0
    assert np.abs(tr.buf.double().cpu().numpy() - buf).max() <= (tol.cpu().numpy() + 4 * 2.0 ** -24 * np.abs(buf)).max()


def _train8(seed_batch=1):
    from torchdet3d.trainer import DetectorHeadTrainer
    det = _det(torch.bfloat16)
    batch = _batch(2, (2, 2), seed=seed_batch)
    before = det.loss(*batch)
    before = (before['loss_cls'] + before['loss_bbox']).item()
    tr = DetectorHeadTrainer(det, warmup_iters=4)
    losses = []
    for _ in range(8):
        losses.append(tr.train_step(*batch)[2])
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
    # the eval path folded the trained parameters and moved running statistics again
    assert np.isfinite(after) and after != before


def test_a_recorded_head_backward_replays():
    """head_backward recorded into a plan and replayed gives a fresh call's hgrad bit for bit (the running statistics move in
    both, by the same batch)."""
    N = _N()
    det = _det(torch.bfloat16)
    batch = _batch(2, (1, 3), seed=2)
    det.head_backward(*batch, tap_grads=True)              # (buffers exist, the backbone's packs are made)
    torch.cuda.synchronize()
    rec = N.PlanRecorder()
    N.recorder = rec
    try:
        r = det.head_backward(*batch, tap_grads=True)
        rec.end_segment()
    finally:
        N.recorder = None
    try:
        torch.cuda.synchronize()
        assert rec.broken is None
        recorded = det.hgrad.clone()
        for v in det.hg.values():              # (not the flat buffer: the call never writes its pads, they stay zero)
            v.fill_(float('nan'))
        for t in r['dtaps']:
            t.fill_(float('nan'))
        slots = (ctypes.c_ulonglong * N.NSLOTS)()
        assert N.lib().t3d_plan_run(rec.plan, 0, slots, N.NSLOTS, None, 0) >= 0
        torch.cuda.synchronize()
        replayed, dt_replayed, loss_replayed = det.hgrad.clone(), [t.clone() for t in r['dtaps']], r['loss_cls'].item()
        fresh = det.head_backward(*batch, tap_grads=True)
        torch.cuda.synchronize()
        assert torch.isfinite(replayed).all() and (replayed != 0).any()
        assert torch.equal(replayed.view(torch.int32), det.hgrad.view(torch.int32))
        assert torch.equal(replayed.view(torch.int32), recorded.view(torch.int32))
        for a, b in zip(dt_replayed, fresh['dtaps']):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert loss_replayed == fresh['loss_cls'].item()
    finally:
        rec.close()
