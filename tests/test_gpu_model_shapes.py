"""GPU parity of the whole fp32 model off the square grid and at the reference's per-replica batch, against the CPU oracle
on identical weights and crops (the checks of tests/test_gpu_engine.py at new shapes).

Kernel choice happens at model level and depends on H and W separately (the two-column / second-row paths of the 3x3
depthwise stream, the 7x7-plane special case of the depthwise forward and backward, the sample-boundary path of the
pointwise GEMM), and on the batch against the tile sizes.  The cases reach: W != H in every depthwise / pointwise dispatch
(160 x 128); odd planes after every stride 2 (100 -> 50 -> 25 -> 13 -> 7 -> 4); W > H with a 5x5 depthwise on a 3 x 5 last
plane; and B = 82 = 2 * 41, what each of the reference's two replicas sees of its train batch of 164."""
import numpy as np
import pytest
import torch

from test_gpu_engine import ELEM_TOL, L2_TOL, _loss_cfg, _oracle_step

pytestmark = pytest.mark.gpu

LNAMES, COEFFS, NC = ['l1', 'add_loss', 'cross_entropy'], ([1., .1], [.2]), 9

# (name, B, H, W, gradient gate): 'small' is test_train_step_fp32_matches_oracle's (ELEM_TOL / L2_TOL or 3x the fp32
# oracle's own distance from fp64), 'headline' that of
# test_headline_model_backward_against_the_fp64_oracle_at_production_resolution (1.5e-2 / 1e-2 or 2.5x)
CASES = [('mobilenetv2', 12, 160, 128, 'kinked'),
         ('mobilenetv3_small', 9, 100, 100, 'small'),
         ('mobilenetv3_large', 6, 96, 160, 'small'),
         ('mobilenetv3_large', 82, 224, 224, 'headline')]
# 'kinked': the small-batch gate with absolute terms 1.5x wider.  At mobilenetv2 B = 12 @160x128 the FP64 oracle itself moves
# `features.10.conv.1.bias` (a depthwise BatchNorm bias of the 10 x 8 stage) by 1.03e-1 of its largest entry and 2.4e-2 of its
# norm when the crops get 1e-6 relative noise (a ReLU6 kink flips); the HIP path sits at 1.02e-1 / 2.1e-2 there, every other
# tensor inside ELEM_TOL / L2_TOL.
GATES = {'small': (ELEM_TOL, L2_TOL, 3.0), 'kinked': (1.5 * ELEM_TOL, 1.5 * L2_TOL, 3.0), 'headline': (1.5e-2, 1e-2, 2.5)}


def _grad_gate(tag, got, grads_o, grads_64, gate):
    """Every weight gradient of the HIP path against the fp64 oracle, with the fp32 oracle's own distance from it as the
    conditioning yardstick (relative to the tensor's largest entry element-wise, to its norm in L2)."""
    elem_tol, l2_tol, k_ref = GATES[gate]
    bad, worst = [], [0.0, 0.0, 0.0, 0.0]
    for k, g64 in grads_64.items():
        g = got[k].cpu().double()
        scale = max(g64.abs().max().item(), 1e-3)
        nrm = max(g64.norm().item(), 1e-3 * g64.numel() ** .5)
        err, err_ref = (g - g64).abs().max().item() / scale, (grads_o[k].double() - g64).abs().max().item() / scale
        l2, l2_ref = (g - g64).norm().item() / nrm, (grads_o[k].double() - g64).norm().item() / nrm
        worst = [max(worst[0], err), max(worst[1], err_ref), max(worst[2], l2), max(worst[3], l2_ref)]
        if not (err < max(elem_tol, k_ref * err_ref) and l2 < max(l2_tol, k_ref * l2_ref)):
            bad.append((k, err, err_ref, l2, l2_ref))
    print(f'[grad gate {tag}, {gate}] worst max-norm error HIP {worst[0]:.3e} / oracle fp32 {worst[1]:.3e}; '
          f'worst relative L2 HIP {worst[2]:.3e} / oracle fp32 {worst[3]:.3e} (all against the fp64 oracle, '
          f'{len(grads_64)} tensors)')
    assert not bad, bad[:10]


@pytest.mark.parametrize('name,B,H,W,gate', CASES)
def test_model_matches_the_oracle_off_the_square_grid(name, B, H, W, gate):
    import time
    from oracle import model as OMod
    from oracle.weights import make_inputs, make_state_dict
    from torchdet3d import _native as N
    from torchdet3d.models.arch import Arch
    from torchdet3d.models.engine import Net
    tag = f'{name} B={B} @{H}x{W}'
    sd = make_state_dict(name, NC)
    imgs, gt_kp, cats = make_inputs(B, H, W, NC)
    mask = (torch.rand(B, Arch(name).feat_c, generator=torch.Generator().manual_seed(3)) >= 0.5).float() * 2
    net = Net(name, NC, 'cuda', torch.float32)
    net.load_state_dict(sd)
    # eval forward
    with torch.no_grad():
        kp_o, tg_o = OMod.forward(sd, name, imgs, cats, train=False, num_classes=NC)
    kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=False)
    np.testing.assert_allclose(kp.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(lg.cpu().numpy(), tg_o.numpy(), atol=1e-4)
    assert (lg.argmax(1).cpu() == tg_o.argmax(1)).all()
    # train step: oracle in fp32 and fp64, HIP forward with the same dropout mask, fused losses, backward
    t0 = time.time()
    kp_o, tg_o, loss_o, grads_o, params_o = _oracle_step(name, sd, imgs, gt_kp, cats, NC, LNAMES, COEFFS, mask)
    t1 = time.time()
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    grads_64 = _oracle_step(name, sd64, imgs.double(), gt_kp.double(), cats, NC, LNAMES, COEFFS, mask.double())[3]
    print(f'[{tag}] oracle train step on {torch.get_num_threads()} threads: fp32 {t1 - t0:.1f} s, fp64 {time.time() - t1:.1f} s')
    kp, lg = net.forward(imgs.cuda(), cats.cuda(), train=True, dropout_mask=mask.cuda())
    np.testing.assert_allclose(kp.cpu().numpy(), kp_o.numpy(), atol=1e-4)
    np.testing.assert_allclose(lg.cpu().numpy(), tg_o.numpy(), atol=1e-4)
    out = torch.zeros(16, device='cuda')
    dkp, dlg = torch.empty(B, 18, device='cuda'), torch.empty(B, NC, device='cuda')
    gtd, cd = gt_kp.cuda().view(B, 18).contiguous(), cats.cuda()
    N.call('t3d_loss_fwd_bwd', _loss_cfg(LNAMES, COEFFS), N.ptr(kp.view(B, 18)), N.ptr(gtd), N.ptr(lg), N.ptr(cd), N.ptr(out),
           N.ptr(dkp), N.ptr(dlg), B, NC, N.stream())
    np.testing.assert_allclose(out[0].item(), loss_o.item(), rtol=2e-5)
    net.backward(dkp, dlg)
    torch.cuda.synchronize()
    _grad_gate(tag, net.g, grads_o, grads_64, gate)
    # BatchNorm running statistics (the first and the last BatchNorm, as test_train_step_fp32_matches_oracle)
    for k in ('features.0.1', 'conv.1'):
        np.testing.assert_allclose(net.buffers[k + '.running_mean'].cpu().numpy(),
                                   params_o[k + '.running_mean'].numpy(), atol=1e-5)
        np.testing.assert_allclose(net.buffers[k + '.running_var'].cpu().numpy(),
                                   params_o[k + '.running_var'].numpy(), rtol=1e-4, atol=1e-6)
        assert int(net.buffers[k + '.num_batches_tracked']) == int(params_o[k + '.num_batches_tracked'])


def test_uint8_crops_off_the_square_grid_match_the_normalised_fp32_path():
    """NHWC uint8 crops of 160 x 128 through the model (normalisation fused into the stem's patch gather) against the fp32
    path on the normalised crops, with the bounds of test_gpu_stem.py's 128 x 128 case."""
    from test_gpu_stem import uint8_crops_match_the_fp32_path
    uint8_crops_match_the_fp32_path(160, 128)
