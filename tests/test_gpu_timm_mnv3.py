"""'mobilenetv3_large_21k' on the GPU against the test-side restatement (tests/timm_mnv3_ref.py; the frozen oracle does not
know the name): fp32 parity of the eval forward and the whole train step with the gates of tests/test_gpu_engine.py, bf16
training, the step plan, Trainer / Evaluator, checkpoints, the inference engines."""
import os

import numpy as np
import pytest
import torch

import timm_mnv3_ref as R
from test_gpu_engine import ELEM_TOL, L2_TOL, _loss_cfg
from test_host_logic import _cfg

pytestmark = pytest.mark.gpu
NAME = R.NAME
STEM_BN, LAST_BN, LAST_W = 'model.bn1', 'model.blocks.6.0.bn1', 'model.blocks.6.0.conv.weight'


def _inputs(B, S, nc):
    from oracle.weights import make_inputs
    H, W = S if isinstance(S, tuple) else (S, S)
    return make_inputs(B, H, W, nc)


def _ref_step(sd, imgs, gt_kp, cats, nc, lnames, coeffs, mask, pooling_mode='avg'):
    """One train step of the restatement (the dtype of `sd` / `imgs` decides the precision) -> kp, logits, loss, grads, params."""
    from oracle import losses as OL
    params = {k: v.clone().requires_grad_(v.dtype.is_floating_point and 'running' not in k) for k, v in sd.items()}
    kp, tg = R.forward(params, imgs, cats, train=True, num_classes=nc, dropout_mask=mask, pooling_mode=pooling_mode)
    lm = OL.LossManager(OL.build(lnames), coeffs)
    loss = lm.parse_losses(kp, gt_kp, tg, cats, 0)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in params.items() if v.requires_grad}
    return kp.detach(), (tg.detach() if nc > 1 else None), loss.detach().reshape(-1), grads, params


def _hip_step(net, imgs, gt_kp, cats, nc, lnames, coeffs, mask):
    from torchdet3d import _native as N
    B = imgs.shape[0]
    kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=True, dropout_mask=mask.cuda() if mask is not None else None)
    out = torch.zeros(16, device='cuda')
    dkp = torch.empty(B, 18, device='cuda')
    dlg = torch.empty(B, nc, device='cuda') if nc > 1 else None
    gtd, cd = gt_kp.cuda().view(B, 18).contiguous(), cats.cuda()
    N.call('t3d_loss_fwd_bwd', _loss_cfg(lnames, coeffs), N.ptr(kp.view(B, 18)), N.ptr(gtd), N.ptr(lg), N.ptr(cd), N.ptr(out),
           N.ptr(dkp), N.ptr(dlg), B, nc, N.stream())
    return kp, lg, out, dkp, dlg


CASES = [(4, 96, 9, ['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2]), 'avg'),
         (2, 224, 9, ['smoothl1', 'wing', 'cross_entropy'], ([1., .3], [.5]), 'avg'),
         (6, 128, 1, ['mse', 'diag_loss', 'add_loss'], ([1., .5, .1], []), 'avg'),
         (3, (160, 128), 9, ['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2]), 'avg'),
         # + the doubled features of the wrapper's 'avg+max' pool over the head's 1x1 map, through the backward
         (4, 96, 9, ['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2]), 'avg+max')]


@pytest.mark.parametrize('B,S,nc,lnames,coeffs,pmode', CASES,
                         ids=['b4-96', 'b2-224', 'b6-128-nc1', 'b3-160x128', 'b4-96-avg+max'])
def test_fp32_eval_and_train_step_match_the_restatement(B, S, nc, lnames, coeffs, pmode):
    from torchdet3d.models.engine import Net
    sd = R.make_state_dict(nc)
    imgs, gt_kp, cats = _inputs(B, S, nc)
    mask = (torch.rand(B, 1280, generator=torch.Generator().manual_seed(3)) >= 0.5).float() * 2 if nc > 1 else None
    net = Net(NAME, nc, 'cuda', torch.float32, pmode)
    net.load_state_dict(sd)
    # ---- eval forward
    with torch.no_grad():
        kp_o, tg_o = R.forward(sd, imgs, cats, train=False, num_classes=nc, pooling_mode=pmode)
    kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=False)
    print(f'[eval {pmode}] max |dkp| {(kp.cpu() - kp_o).abs().max().item():.2e}')
    np.testing.assert_allclose(kp.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    if nc > 1:
        np.testing.assert_allclose(lg.cpu().numpy(), tg_o.numpy(), atol=1e-4)
        assert (lg.argmax(1).cpu() == tg_o.argmax(1)).all()
    # ---- train step
    kp_o, tg_o, loss_o, grads_o, params_o = _ref_step(sd, imgs, gt_kp, cats, nc, lnames, coeffs, mask, pmode)
    grads_64 = _ref_step(R.cast(sd, torch.float64), imgs.double(), gt_kp.double(), cats, nc, lnames, coeffs,
                         mask.double() if mask is not None else None, pmode)[3]
    kp, lg, out, dkp, dlg = _hip_step(net, imgs, gt_kp, cats, nc, lnames, coeffs, mask)
    np.testing.assert_allclose(kp.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    if nc > 1:
        np.testing.assert_allclose(lg.cpu().numpy(), tg_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(out[0].item(), loss_o.item(), rtol=2e-5)
    net.backward(dkp, dlg)
    torch.cuda.synchronize()
    bad, worst = [], [0.0, 0.0]
    for k, g64 in grads_64.items():
        got = net.g[k].cpu().double()
        scale = max(g64.abs().max().item(), 1e-3)
        err = (got - g64).abs().max().item() / scale
        err_ref = (grads_o[k].double() - g64).abs().max().item() / scale
        nrm = max(g64.norm().item(), 1e-3 * g64.numel() ** .5)
        l2 = (got - g64).norm().item() / nrm
        l2_ref = (grads_o[k].double() - g64).norm().item() / nrm
        worst[0], worst[1] = max(worst[0], err if err >= 3 * err_ref else 0.0), max(worst[1], l2 if l2 >= 3 * l2_ref else 0.0)
        if not (err < max(ELEM_TOL, 3 * err_ref) and l2 < max(L2_TOL, 3 * l2_ref)):
            bad.append((k, err, err_ref, l2, l2_ref, scale))
    print(f'[grad gate {NAME} B={B} @{S} {pmode}] worst element-wise / L2 error where the absolute term binds: '
          f'{worst[0]:.3e} / {worst[1]:.3e}')
    assert not bad, bad[:10]
    assert set(grads_64) == set(net.g)
    for k in (STEM_BN, LAST_BN, 'model.blocks.4.1.bn2'):
        np.testing.assert_allclose(net.buffers[k + '.running_mean'].cpu().numpy(), params_o[k + '.running_mean'].numpy(), atol=1e-5)
        np.testing.assert_allclose(net.buffers[k + '.running_var'].cpu().numpy(), params_o[k + '.running_var'].numpy(),
                                   rtol=1e-4, atol=1e-5)
        assert int(net.buffers[k + '.num_batches_tracked']) == int(params_o[k + '.num_batches_tracked'])


@pytest.mark.parametrize('pmode', ['avg', 'max', 'avg+max'])
def test_every_pooling_mode_in_eval_export_mode_and_uint8_crops(pmode):
    from torchdet3d.builders import build_model
    nc, B, S = 9, 4, 96
    sd = R.make_state_dict(nc)
    imgs, _, cats = _inputs(B, S, nc)
    cfg = _cfg(NAME)
    cfg.model.pooling_mode = pmode
    m = build_model(cfg)
    m.load_state_dict(sd)
    m.to('cuda').eval()
    with torch.no_grad():
        kp_o, tg_o = R.forward(sd, imgs, cats, num_classes=nc, pooling_mode=pmode)
        kp, tg = m(imgs.cuda(), cats.cuda())
    np.testing.assert_allclose(kp.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(tg.cpu().numpy(), tg_o.numpy(), atol=1e-4)
    assert (tg.argmax(1).cpu() == tg_o.argmax(1)).all()
    # export mode: all nine heads on every sample (forward_to_onnx)
    me = build_model(cfg, export_mode=True)
    me.load_state_dict(sd)
    me.to('cuda').eval()
    with torch.no_grad():
        kp9_o, tg9_o = R.forward_to_onnx(sd, imgs, nc, pooling_mode=pmode)
        kp9, tg9 = me(imgs.cuda())
    assert kp9.shape == (9, B, 9, 2)
    np.testing.assert_allclose(kp9.cpu().numpy(), kp9_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(tg9.cpu().numpy(), tg9_o.numpy(), atol=1e-4)
    # uint8 NHWC crops, normalised inside the stem's patch gather
    u8 = torch.randint(0, 256, (B, S, S, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    mean, std = (torch.tensor(v) for v in m.input_normalization)
    x = ((u8.float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        kp_o, tg_o = R.forward(sd, x, cats, num_classes=nc, pooling_mode=pmode)
        kp, tg = m(u8.cuda(), cats.cuda())
    np.testing.assert_allclose(kp.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(tg.cpu().numpy(), tg_o.numpy(), atol=1e-4)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_one_launch_gate_backward_and_the_sequence_agree_on_the_same_forward(dtype, monkeypatch):
    """The engine's two paths for the gate-after backward (t3d_se_after_bwd / the three launches) on ONE saved forward: the
    same gradients up to summation order in fp32 storage (1e-4 of a tensor's largest entry; measured value printed), and up
    to the bf16 quantisation floor of a re-rounded gradient chain in bf16 storage (the yardstick of
    tests/test_gpu_engine.py::test_yfree_expand_backward_matches_regular_path: total 3e-2)."""
    from torchdet3d.models import engine as E
    B, S, nc = 8, 96, 9
    imgs, gt_kp, cats = _inputs(B, S, nc)
    net = E.Net(NAME, nc, 'cuda', dtype)
    net.reset_parameters(seed=11)
    lnames, coeffs = ['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2])
    kp, lg, out, dkp, dlg = _hip_step(net, imgs, gt_kp, cats, nc, lnames, coeffs, torch.ones(B, 1280))
    saved, grads, launches = net.saved, [], []
    from torchdet3d import _native as N
    for fused in (False, False, True):        # (the first pass also registers the backward's scratch: not counted)
        monkeypatch.setattr(E, 'SE_AFTER_FUSED', fused)
        net.saved = saved
        net._statbuf[:, net._statbuf.shape[1] // 2:].zero_()      # the backward sums of the previous pass
        n0 = N.launch_count()
        net.backward(dkp, dlg)
        torch.cuda.synchronize()
        launches.append(N.launch_count() - n0)
        grads.append({k: v.detach().double().cpu().clone() for k, v in net.g.items()})
    _, seq, one = grads
    assert launches[1] - launches[2] == 8 * 3, launches          # 8 gated blocks: 4 kernels (sums, 2 FC slices, apply) -> 1
    tot = sum((one[k] - seq[k]).norm().item() ** 2 for k in seq) ** .5 / sum(seq[k].norm().item() ** 2 for k in seq) ** .5
    worst = max(((one[k] - seq[k]).abs().max().item() / max(seq[k].abs().max().item(), 1e-3), k) for k in seq)
    print(f'[{dtype}] one launch vs sequence on the same forward: total relative L2 {tot:.3e}, worst tensor (max-norm) {worst}')
    if dtype == torch.float32:
        assert worst[0] < 1e-4, worst
    else:
        assert tot < 3e-2, tot


def test_bf16_train_step_close_to_the_restatement():
    """The loose bounds of tests/test_gpu_engine.py::test_train_step_bf16_close_to_oracle."""
    from torchdet3d.models.engine import Net
    B, S, nc = 32, 96, 9
    lnames, coeffs = ['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2])
    net = Net(NAME, nc, 'cuda', torch.bfloat16)
    net.reset_parameters(seed=11)
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    imgs, gt_kp, cats = _inputs(B, S, nc)
    kp_o, tg_o, loss_o, grads_o, _ = _ref_step(sd, imgs, gt_kp, cats, nc, lnames, coeffs, None)
    kp, lg, out, dkp, dlg = _hip_step(net, imgs, gt_kp, cats, nc, lnames, coeffs, torch.ones(B, 1280))
    print(f'bf16 train step: max |dkp| {(kp.cpu() - kp_o).abs().max().item():.2e} loss {out[0].item():.5f} / {loss_o.item():.5f}')
    assert (kp.cpu() - kp_o).abs().max() < 5e-2
    assert abs(out[0].item() - loss_o.item()) < 5e-2 * abs(loss_o.item())
    net.backward(dkp, dlg)
    for k in ('regressors.0.0.weight', 'cls_fc.1.weight', LAST_W):
        a, b = net.g[k].cpu().flatten().double(), grads_o[k].flatten().double()
        cos = ((a @ b) / (a.norm() * b.norm() + 1e-30)).item()
        assert cos > 0.8, (k, cos)


@pytest.mark.parametrize('fused', [None, True, False], ids=['by-shape', 'one-launch', 'sequence'])
@pytest.mark.parametrize('B,S', [(16, 96), (32, 224)])
def test_bf16_training_is_bit_reproducible_run_to_run(B, S, fused, monkeypatch):
    """Three optimizer steps through the reference-shaped API, run twice from the same seed: identical losses, gradients
    and weights, bit for bit -- with the gate-after backward chosen by shape, forced to the one launch, forced to the
    sequence."""
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.models import engine as E
    monkeypatch.setattr(E, 'SE_AFTER_FUSED', fused)
    imgs, gt_kp, cats = (t.cuda() for t in _inputs(B, S, 9))
    cfg = _cfg(NAME)
    cfg.model.storage_dtype = 'bf16'
    sd = R.make_state_dict(9)

    def run():
        torch.manual_seed(3)
        m = build_model(cfg)
        m.load_state_dict(sd)
        m.to('cuda')
        m.train()
        opt = build_optimizer(cfg, m)
        lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
        gen = torch.Generator(device='cuda').manual_seed(5)
        trace = []
        for it in range(3):
            mask = (torch.rand(B, 1280, device='cuda', generator=gen) > 0.2).float() * 1.25
            kp, tg = m(imgs, cats, dropout_mask=mask)
            loss = lm.parse_losses(kp, gt_kp, tg, cats, it)
            opt.zero_grad()
            loss.backward()
            trace.append((loss.detach().clone(), m.net.gflat.clone()))
            opt.step()
        torch.cuda.synchronize()
        return trace, m.net.flat.clone()

    (ta, wa), (tb, wb) = run(), run()
    for it, ((la, ga), (lb, gb)) in enumerate(zip(ta, tb)):
        assert torch.isfinite(la).all()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        assert torch.equal(ga, gb), (it, (ga - gb).abs().max().item())
    assert torch.equal(wa, wb)


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_step_plan_replay_is_bit_identical_to_the_eager_step(optim):
    from test_gpu_fused_optimizers import _run, _same
    steps = 7
    eager = _run(NAME, 'bf16', optim, 16, 96, steps, 'eager', lr_at=5)
    direct = _run(NAME, 'bf16', optim, 16, 96, steps, 'direct', lr_at=5)
    replay = _run(NAME, 'bf16', optim, 16, 96, steps, 'replay', lr_at=5)
    _same(eager, direct)
    _same(eager, replay)
    sp = replay[4]._sp
    assert sp is not None and sp.rec is not None and sp.replays == steps - 3      # two warm steps, one recorded, the rest replayed
    assert eager[4]._sp is None
    names = [c[0] for c in sp.rec.calls]
    assert names.count('t3d_se_after_bwd') + names.count('t3d_se_after_apply') == 8      # every gated block's backward is in the plan
    assert names.count('t3d_gap_fwd') == 8


def test_trainer_evaluator_and_checkpoints_through_build_model(tmp_path):
    from torchdet3d.builders import build_loader, build_loss, build_model, build_optimizer, build_scheduler
    from torchdet3d.evaluation import Evaluator
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    from torchdet3d.utils import load_pretrained_weights, resume_from, save_snap
    cfg = _cfg(NAME)
    cfg.data.update(root='synthetic', resize=(96, 96), train_batch_size=16, val_batch_size=16, synthetic_len=64)
    train_loader, val_loader, _ = build_loader(cfg)
    net = build_model(cfg).to('cuda')
    opt = build_optimizer(cfg, net)
    sched = build_scheduler(cfg, opt)

    class W:                      # SummaryWriter stand-in
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, v, global_step=None):
            self.rows.append((tag, float(v), global_step))

    w = W()
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    tr = Trainer(model=net, train_loader=train_loader, optimizer=opt, scheduler=sched, loss_manager=lm, writer=w,
                 max_epoch=3, log_path=str(tmp_path), device='cuda', save_chkpt=True, debug=False, save_freq=10,
                 print_freq=100, train_step=0)
    first = tr.train(0, False)['loss']
    tr.train(1, False)
    last = tr.train(2, True)['loss']
    assert np.isfinite(last) and last < first, (first, last)          # it learns the synthetic set
    assert tr.global_step == 12 and os.path.exists(tmp_path / 'snap_2.pth')
    ev = Evaluator(model=net, val_loader=val_loader, cfg=cfg, writer=w, max_epoch=3, device='cuda')
    res = ev.val(epoch=2, compute_iou=True)
    assert 0 <= res['ADD'] <= 2 and 0 <= res['IOU'] <= 1 and 0 <= res['ACC'] <= 1
    # state_dict -> load_state_dict round trip (new keys, conv-shaped squeeze-excite weights)
    sd = net.state_dict()
    assert list(sd) == list(R.state_dict_shapes(9)) and sd['model.blocks.5.0.se.conv_expand.weight'].shape == (672, 168, 1, 1)
    m2 = build_model(cfg).to('cuda')
    m2.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    imgs, gt_kp, cats = next(iter(val_loader))
    net.eval(), m2.eval()
    with torch.no_grad():
        a, b = net(imgs.cuda(), cats.cuda()), m2(imgs.cuda(), cats.cuda())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # save_snap / resume_from / load_pretrained_weights with the new keys
    save_snap(net, opt, sched, 7, str(tmp_path))
    m3 = build_model(cfg).to('cuda')
    opt3 = build_optimizer(cfg, m3)
    assert resume_from(m3, str(tmp_path / 'snap_7.pth'), opt3, build_scheduler(cfg, opt3)) == 8
    assert all(torch.equal(v, sd[k]) for k, v in m3.state_dict().items())
    cfg.model.load_weights = str(tmp_path / 'snap_7.pth')
    m4 = build_model(cfg)
    assert all(torch.equal(v.cpu(), sd[k].cpu()) for k, v in m4.state_dict().items())
    m5 = load_pretrained_weights(build_model(_cfg(NAME)), pretrained_dict={'module.' + k: v for k, v in sd.items()})
    assert torch.equal(m5.state_dict()[LAST_W].cpu(), sd[LAST_W].cpu())


def _metrics_distance(kp, lg, kp32, gt_kp, cats):
    from test_gpu_bf16_gate import _gt_star, _iou, _metrics
    a, s, acc = _metrics(kp, gt_kp.cuda(), lg, cats.cuda())
    a32, s32, _ = _metrics(kp32, gt_kp.cuda(), lg, cats.cuda())
    d = (kp - kp32).cpu()
    ious = []
    for sigma in (0.01, 0.024, 0.05):
        gts = _gt_star(kp32.cpu().numpy(), sigma)
        ious.append((sigma, _iou(kp.cpu(), gts) - _iou(kp32.cpu(), gts)))
    return (f'keypoints rms {d.pow(2).mean().sqrt().item():.2e} max {d.abs().max().item():.2e}; dADD {a - a32:+.2e} dSADD {s - s32:+.2e}; '
            + ' '.join(f'd3-D-IoU(sigma {sg}) {v:+.2e}' for sg, v in ious))


def test_inference_engines_at_b32_224():
    """The default inference engine (fp32 storage, also under a bf16-trained model) meets the 1e-4 / arg-max gate at
    B = 32 @224^2; the f16 and bf16 engines run, give finite outputs and agree with it on the class arg-max.  Their
    keypoint / ADD / 3-D-IoU distance from the fp32 engine is PRINTED (recorded in DESIGN.md), not gated: whether a 16-bit
    engine of this model is inside the 1e-3 bound is a measurement, not a promise (mobilenetv2's bf16 engine is not,
    tests/test_gpu_bf16_gate.py)."""
    from torchdet3d.builders import build_model
    from torchdet3d.models.engine import Net
    B, S, nc = 32, 224, 9
    sd = R.make_state_dict(nc)
    imgs, gt_kp, cats = _inputs(B, S, nc)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        kp_o, tg_o = R.forward(sd, imgs, cats, num_classes=nc)
    cfg = _cfg(NAME)
    cfg.model.storage_dtype = 'bf16'
    m = build_model(cfg)
    m.load_state_dict(sd)
    m.to('cuda').eval()
    assert m.net.dtype == torch.bfloat16 and m.net_eval is not m.net and m.net_eval.dtype == torch.float32
    with torch.no_grad():
        kp32, lg32 = m(imgs.cuda(), cats.cuda())
    kp32, lg32 = kp32.clone(), lg32.clone()
    print(f'fp32 engine b32@224: max |dkp| {(kp32.cpu() - kp_o).abs().max().item():.2e} max |dlogit| {(lg32.cpu() - tg_o).abs().max().item():.2e}')
    np.testing.assert_allclose(kp32.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(lg32.cpu().numpy(), tg_o.numpy(), atol=1e-4)
    assert (lg32.argmax(1).cpu() == tg_o.argmax(1)).all()
    for evdt, tdt in (('f16', torch.float16), ('bf16', torch.bfloat16)):
        cfg.model.eval_storage_dtype = evdt
        me = build_model(cfg)
        me.load_state_dict(sd)
        me.to('cuda').eval()
        assert me.net_eval.dtype == tdt
        with torch.no_grad():
            kp, lg = me(imgs.cuda(), cats.cuda())
        kp, lg = kp.clone(), lg.clone()
        assert torch.isfinite(kp).all() and torch.isfinite(lg).all()
        print(f'{evdt} engine b32@224 vs the fp32 engine: {_metrics_distance(kp.view(B, 9, 2), lg, kp32.view(B, 9, 2), gt_kp, cats)}; '
              f'max |dlogit| {(lg - lg32).abs().max().item():.2e}')
        assert (lg.argmax(1) == lg32.argmax(1)).all()
        net = Net(NAME, nc, 'cuda', tdt)
        if tdt == torch.float16:
            with pytest.raises(RuntimeError, match='inference-only'):
                net.forward(imgs.cuda()[:8], cats.cuda()[:8], train=True)
