"""GPU: `t3d_augment_crops_u8` (csrc/augment.hip) bit-exact against the numpy restatement of the reference's crop
pipeline (tests/augment_ref.py): identity (also == t3d_crop_resize_u8 and oracle resize_linear_u8), flip, LUT, rotate,
all combined, channel swap, crop sizes around the output size, 1-pixel crops, a non-square output, B = 1 and B = 257."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu


def _run(crops, prm, oh, ow):
    """crops: list of uint8 [h, w, 3]; prm: list of dicts (flip, alpha, beta, angle, swap) -> uint8 [B, oh, ow, 3]."""
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    B = len(crops)
    rec = np.zeros(B, AUG_SAMPLE_DTYPE)
    parts, off = [], 0
    for i, (c, p) in enumerate(zip(crops, prm)):
        rec['offset'][i], rec['h'][i], rec['w'][i] = off, c.shape[0], c.shape[1]
        parts.append(c.reshape(-1))
        off += c.size
        fl = 0
        if p.get('flip'):
            fl |= 1
        if p.get('alpha', 1.0) != 1.0 or p.get('beta', 0.0) != 0.0:
            fl |= 2
            rec['alpha'][i], rec['beta255'][i] = np.float32(p.get('alpha', 1.0)), np.float32(p.get('beta', 0.0) * 255)
        if p.get('angle') is not None:
            fl |= 4
            rec['m'][i] = R.invert_affine(R.rotation_matrix(p['angle'], oh, ow)).reshape(-1)
        if p.get('swap'):
            fl |= 8
        rec['flags'][i] = fl
    src = torch.from_numpy(np.concatenate(parts)).cuda()
    recd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    out = torch.full((B, oh, ow, 3), 77, dtype=torch.uint8, device='cuda')
    N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(recd), N.ptr(out), B, oh, ow, N.stream())
    return out.cpu().numpy()


def _check(crops, prm, oh, ow):
    got = _run(crops, prm, oh, ow)
    for i, (c, p) in enumerate(zip(crops, prm)):
        ref = R.augment(c, oh, ow, p.get('flip', False), p.get('alpha', 1.0), p.get('beta', 0.0), p.get('angle'),
                        p.get('swap', False))
        assert np.array_equal(got[i], ref), (i, c.shape, p, np.abs(got[i].astype(int) - ref.astype(int)).max())
    return got


def _crops(rng, n, lo=150, hi=500, smooth=True):
    out = []
    for _ in range(n):
        h, w = rng.integers(lo, hi, 2)
        c = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if smooth:
            yy, xx = np.mgrid[0:h, 0:w]
            c = np.clip(np.stack([127 + 110 * np.sin(xx / 13. + k) * np.cos(yy / 17. - k) for k in range(3)], -1)
                        + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)
        out.append(c)
    return out


def test_identity_equals_crop_resize_and_the_oracle():
    from oracle.crop_resize import resize_linear_u8
    from torchdet3d import _native as N
    rng = np.random.default_rng(0)
    H, W = 480, 640
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rects = np.array([[0, 0, W, H], [10, 20, 11, 300], [5, 5, 400, 6], [100, 50, 250, 450], [3, 3, 227, 227],
                      [600, 400, 640, 480]], np.int32)
    crops = [frame[y0:y1, x0:x1] for x0, y0, x1, y1 in rects]
    got = _check(crops, [{}] * len(crops), 224, 224)
    out = torch.zeros(len(rects), 224, 224, 3, dtype=torch.uint8, device='cuda')
    fd, rd = torch.from_numpy(frame).cuda(), torch.from_numpy(rects).cuda()
    N.call('t3d_crop_resize_u8', N.ptr(fd), N.ptr(rd), N.ptr(out), len(rects), H, W, 224, 224, N.stream())
    assert np.array_equal(got, out.cpu().numpy())
    for g, c in zip(got, crops):
        assert np.array_equal(g, resize_linear_u8(c, (224, 224)))


@pytest.mark.parametrize('case', ['flip', 'lut', 'rot0', 'rot+10', 'rot-10', 'rot1e-3', 'all', 'swap'])
def test_each_step_bit_exact(case):
    rng = np.random.default_rng(hash(case) % 1000)
    crops = _crops(rng, 6) + _crops(rng, 2, smooth=False)
    p = dict(flip={'flip': True}, lut={'alpha': 1.17, 'beta': -0.13}, rot0={'angle': 0.0}, swap={'swap': True},
             all={'flip': True, 'alpha': 0.83, 'beta': 0.19, 'angle': -7.3, 'swap': True})
    p.update({'rot+10': {'angle': 10.0}, 'rot-10': {'angle': -10.0}, 'rot1e-3': {'angle': 1e-3}})
    _check(crops, [p[case]] * len(crops), 224, 224)


def test_lut_saturates_and_matches_albumentations_float32():
    rng = np.random.default_rng(5)
    crops = _crops(rng, 5, smooth=False)
    prm = [{'alpha': 1.2, 'beta': 0.2}, {'alpha': 0.8, 'beta': -0.2}, {'alpha': 1.0, 'beta': 0.2}, {'alpha': 1.2, 'beta': 0.0},
           {'alpha': 0.999, 'beta': 1e-4}]
    _check(crops, prm, 224, 224)


def test_small_large_and_one_pixel_crops_non_square_output():
    rng = np.random.default_rng(7)
    crops = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in
             [(1, 1), (1, 37), (53, 1), (2, 2), (60, 90), (128, 160), (700, 900), (129, 161), (5, 400)]]
    for prm in ({}, {'flip': True, 'alpha': 1.1, 'beta': 0.05, 'angle': 8.0}, {'angle': -3.0, 'swap': True}):
        _check(crops, [prm] * len(crops), 128, 160)
        _check(crops, [prm] * len(crops), 224, 224)


@pytest.mark.parametrize('B', [1, 257])
def test_mixed_batch_in_one_launch(B):
    rng = np.random.default_rng(B)
    crops = _crops(rng, B, 20, 500, smooth=B == 1) if B == 1 else [
        rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(1, 480, (B, 2))]
    prm = []
    for i in range(B):
        u = rng.random(6)
        prm.append(dict(flip=bool(u[0] < .4), alpha=float(1 + .4 * u[1] - .2) if u[2] < .3 else 1.0,
                        beta=float(.4 * u[3] - .2) if u[2] < .3 else 0.0,
                        angle=float(20 * u[4] - 10) if u[5] < .4 else None, swap=bool(i % 3 == 0)))
    _check(crops, prm, 224, 224)
    _check(crops[:min(B, 40)], prm[:min(B, 40)], 7, 5)                   # odd pixel count: the byte-store tail


def test_bad_records_give_zeros_and_arguments_are_checked():
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    rec = np.zeros(2, AUG_SAMPLE_DTYPE)
    rec['h'], rec['w'] = (10, 0), (10, 10)
    rec['offset'] = (100, 0)                               # sample 0 reaches past the buffer, sample 1 is empty
    src = torch.full((300,), 200, dtype=torch.uint8, device='cuda')
    recd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    out = torch.full((2, 8, 8, 3), 77, dtype=torch.uint8, device='cuda')
    N.call('t3d_augment_crops_u8', N.ptr(src), 300, N.ptr(recd), N.ptr(out), 2, 8, 8, N.stream())
    assert (out == 0).all()
    with pytest.raises(RuntimeError):
        N.call('t3d_augment_crops_u8', N.ptr(src), 300, N.ptr(recd), N.ptr(out), 2, 0, 8, N.stream())
