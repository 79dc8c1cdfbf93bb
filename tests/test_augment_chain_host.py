"""CPU: random_rescale, hue_saturation_value and color_jitter in the compiled pipeline (dataloaders/objectron.py) -- the
grammar and its refusals, the old pipeline's draws and records left as they were, the second generator's draws, the chain
records, the keypoints -- and the known answers that keep the numpy restatement (tests/augment_chain_ref.py) honest."""
import itertools

import numpy as np
import pytest

import augment_chain_ref as C
import augment_ref as R

SIZE = (64, 48)
RS = ('random_rescale', dict(scale_limit=(0.8, 1.25), p=0.5))
HSV = ('hue_saturation_value', dict(p=0.5))
CJ = ('color_jitter', dict(p=0.5))


def _pipe(mid, size=SIZE, convert=True):
    from torchdet3d.dataloaders.objectron import AugmentPipeline
    steps = ([('convert_color', dict())] if convert else []) + [('resize', dict(height=size[0], width=size[1]))] + list(mid) + [
        ('normalize', R.NORMALIZATION), ('to_tensor', dict(img_shape=size))]
    return AugmentPipeline(steps, R.NORMALIZATION)


def _default(size=SIZE):
    return R.default_pipelines(size)[0][2:5]          # flip 0.4, brightness / contrast 0.3, rotate 0.4


# ---- compile and refusals ----------------------------------------------------------------------------------------------------
def test_a_pipeline_with_all_three_new_transforms_compiles():
    flip, rbc, rot = _default()
    p = _pipe([HSV, flip, rbc, CJ, RS, rot])
    assert p.chained and p.is_random and p.size == SIZE
    assert p.colour_order == ['hue_saturation_value', 'random_brightness_contrast', 'color_jitter']
    assert p.warp_order == ['random_rescale', 'random_rotate']
    assert (p.p_rescale, p.p_hsv, p.p_jit) == (0.5, 0.5, 0.5) and p.slim == (0.8, 1.25)
    assert p.hsv_lim == ((-20.0, 20.0), (-30.0, 30.0), (-20.0, 20.0))
    assert p.jit_lim == ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.2, 0.2))
    assert _pipe([rot, RS]).warp_order == ['random_rotate', 'random_rescale']
    # the reference's quirk: to_tuple(0.1, bias=0) is (-0.1, 0.1)
    assert _pipe([('random_rescale', dict())]).slim == (-0.1, 0.1)
    assert _pipe([('color_jitter', dict(brightness=1.5, hue=(-0.5, 0.25)))]).jit_lim[::3] == ((0.0, 2.5), (-0.5, 0.25))
    assert not _pipe([('random_rescale', dict(p=0.0))]).is_random and _pipe([('hue_saturation_value', dict(p=0.1))]).is_random
    assert _pipe([('color_jitter', dict(always_apply=True, p=0.0))]).p_jit == 1.0
    assert not _pipe(_default()).chained


@pytest.mark.parametrize('late', ['horizontal_flip', 'random_brightness_contrast', 'hue_saturation_value', 'color_jitter'])
@pytest.mark.parametrize('warp', ['random_rescale', 'random_rotate'])
def test_a_colour_op_or_a_flip_after_a_warp_is_refused(late, warp):
    with pytest.raises(NotImplementedError, match=f'{late} after {warp}'):
        _pipe([(warp, dict()), (late, dict())])


def test_refusals():
    for name in ('blur', 'one_of', 'rgb_shift'):
        with pytest.raises(NotImplementedError, match=name):
            _pipe([(name, dict(p=0.3))])
    with pytest.raises(NotImplementedError, match='times'):
        _pipe([CJ, CJ])
    with pytest.raises(NotImplementedError, match='before resize'):
        from torchdet3d.dataloaders.objectron import AugmentPipeline
        AugmentPipeline([HSV, ('resize', dict(height=8, width=8)), ('normalize', R.NORMALIZATION),
                         ('to_tensor', dict(img_shape=(8, 8)))], R.NORMALIZATION)
    with pytest.raises(NotImplementedError, match='interpolation'):
        _pipe([('random_rescale', dict(interpolation=0))])


@pytest.mark.parametrize('args', [dict(brightness=-0.1), dict(contrast=(-0.5, 1.0)), dict(saturation=(1.2, 0.8)),
                                  dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(hue=-0.1), dict(brightness='x')])
def test_color_jitter_range_errors(args):
    with pytest.raises(ValueError, match='color_jitter'):
        _pipe([('color_jitter', args)])


# ---- the old pipeline is what it was ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', [(5, 0, 0, 0), (5, 3, 1, 17), (0, 0, 0, 0, 12)])
def test_default_pipeline_draws_and_records_are_the_parents(key):
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    p = _pipe(_default())
    n = 9
    prm = p.draw(n, key)
    u = np.random.default_rng(list(key)).random((n, 6))
    want = dict(flip=u[:, 0] < 0.4, lut=u[:, 1] < 0.3, alpha=1.0 + (-0.2 + 0.4 * u[:, 2]), beta=0.0 + (-0.2 + 0.4 * u[:, 3]),
                rot=u[:, 4] < 0.4, angle=-10.0 + 20.0 * u[:, 5])
    assert sorted(prm) == sorted(want)
    for k in want:
        assert prm[k].dtype == want[k].dtype and np.array_equal(prm[k], want[k]), k
    desc = np.stack([np.arange(n) * 30000, np.full(n, 100), np.full(n, 100)], 1).astype(np.int64)
    rec = p.records(desc, prm)
    assert isinstance(rec, np.ndarray) and rec.dtype == AUG_SAMPLE_DTYPE and rec.dtype.itemsize == 80 and rec.shape == (n,)
    assert np.array_equal(rec['flags'], want['flip'] * 1 | want['lut'] * 2 | want['rot'] * 4)
    # the first six columns of a chained pipeline are the same draws
    flip, rbc, rot = _default()
    q = _pipe([flip, rbc, HSV, CJ, RS, rot]).draw(n, key)
    for k in want:
        assert np.array_equal(q[k], want[k]), k


# ---- the new draws ----------------------------------------------------------------------------------------------------------
def test_new_draws_are_deterministic_and_keyed_by_every_component():
    p = _pipe([HSV, CJ, RS])
    new = ('rescale', 'scale', 'hsv', 'dh', 'ds', 'dv', 'jit', 'jb', 'jc', 'js', 'jh', 'order')
    a, b = p.draw(64, (5, 1, 0, 7)), p.draw(64, (5, 1, 0, 7))
    assert all(np.array_equal(a[k], b[k]) for k in a) and set(new) <= set(a)
    assert a['order'].shape == (64, 4) and a['rescale'].dtype == bool and a['scale'].dtype == np.float64
    for other in ((6, 1, 0, 7), (5, 2, 0, 7), (5, 1, 1, 7), (5, 1, 0, 8), (5, 1, 0, 7, 1)):
        c = p.draw(64, other)
        assert all(not np.array_equal(a[k], c[k]) for k in new), other
    assert (a['scale'] >= 0.8).all() and (a['scale'] <= 1.25).all() and (np.abs(a['dh']) <= 20).all()
    assert (np.abs(a['ds']) <= 30).all() and (a['jb'] >= 0.8).all() and (a['jc'] <= 1.2).all() and (np.abs(a['jh']) <= 0.2).all()
    # the second generator equals no generator the loader keys today: its draws are not a continuation of the first's
    u = np.random.default_rng([5, 1, 0, 7]).random((64, 18))
    assert not np.array_equal(a['scale'], 0.8 + 0.45 * u[:, 7])


def test_the_jitter_order_hits_all_24_permutations_and_fires_at_its_rate():
    p = _pipe([CJ])
    d = p.draw(4000, (1, 2, 3, 4))
    orders = {tuple(o) for o in d['order']}
    assert orders == set(itertools.permutations(range(4)))
    assert 0.45 < d['jit'].mean() < 0.55
    counts = np.unique(d['order'] @ (4 ** np.arange(4)), return_counts=True)[1]
    assert counts.min() > 4000 / 24 * 0.6


def test_chain_records():
    from torchdet3d.dataloaders import objectron as O
    flip, rbc, rot = _default()
    p = _pipe([HSV, flip, rbc, CJ, rot, RS], convert=False)
    n = 200
    prm = p.draw(n, (3, 0, 0, 1))
    desc = np.stack([np.arange(n) * 30000, np.full(n, 100), np.full(n, 90)], 1).astype(np.int64)
    rec, ext = p.records(desc, prm)
    assert rec.dtype == O.AUG_SAMPLE_DTYPE and ext.dtype == O.AUG_CHAIN_DTYPE and ext.dtype.itemsize == 280
    oh, ow = SIZE
    seen = set()
    for i in range(n):
        want = [O.CHAIN_HSV] * int(prm['hsv'][i]) + [O.CHAIN_LUT] * int(prm['lut'][i])
        if prm['jit'][i]:
            want += [(O.CHAIN_BRIGHTNESS, O.CHAIN_CONTRAST, O.CHAIN_SATURATION, O.CHAIN_HUE)[k] for k in prm['order'][i]]
        assert ext['n_ops'][i] == len(want) and list(ext['kind'][i, :len(want)]) == want and not ext['kind'][i, len(want):].any()
        assert not rec['flags'][i] & O.AUG_LUT and rec['flags'][i] & O.AUG_SWAP_RB
        assert bool(rec['flags'][i] & O.AUG_FLIP) == prm['flip'][i]
        mats = ([R.rotation_matrix(prm['angle'][i], oh, ow)] if prm['rot'][i] else []) + (
            [C.rescale_matrix(prm['scale'][i], oh, ow)] if prm['rescale'][i] else [])
        assert bool(rec['flags'][i] & O.AUG_ROTATE) == (len(mats) > 0) and ext['flags'][i] == (len(mats) > 1)
        if mats:
            assert np.array_equal(rec['m'][i], R.invert_affine(mats[0]).reshape(-1))
        if len(mats) > 1:
            assert np.array_equal(ext['m2'][i], R.invert_affine(mats[1]).reshape(-1))
        for k, kind in enumerate(want):
            if kind == O.CHAIN_LUT:
                assert tuple(ext['p'][i, k, :2]) == (np.float32(prm['alpha'][i]), np.float32(prm['beta'][i] * 255))
            if kind == O.CHAIN_HSV:
                assert tuple(ext['p'][i, k]) == (prm['dh'][i], prm['ds'][i], prm['dv'][i])
            if kind == O.CHAIN_CONTRAST:
                assert ext['p'][i, k, 0] == prm['jc'][i]
        seen.add((bool(prm['hsv'][i]), bool(prm['jit'][i]), len(mats)))
    assert len(seen) == 12
    assert O.chain_stages(rec, ext) == 7 and O.chain_stages(rec[:0], ext[:0]) == 0
    one = np.zeros(1, O.AUG_CHAIN_DTYPE)
    one['kind'][0, 3] = O.CHAIN_CONTRAST                       # beyond n_ops: not an op
    assert O.chain_stages(np.zeros(1, O.AUG_SAMPLE_DTYPE), one) == 0
    assert O.chain_scratch_bytes(5, 7, 5, 7) == 40 + 2 * 528 and O.chain_scratch_bytes(5, 7, 5, 1) == 40
    # the singular rescale (scale 0, inside the reference's default limits): invert_affine's D == 0 case, a zero map
    assert not O.invert_affine(O.rotation_matrix(0.0, oh, ow, 0.0)).any()


# ---- HSV known answers -------------------------------------------------------------------------------------------------------
def test_hsv_of_primaries_secondaries_greys_and_black():
    rgb = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]], np.uint8)
    hsv = C.rgb_to_hsv_u8(rgb)
    assert hsv[:, 0].tolist() == [0, 30, 60, 90, 120, 150] and (hsv[:, 1:] == 255).all()
    assert np.array_equal(C.hsv_to_rgb_u8(hsv), rgb)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    g = C.rgb_to_hsv_u8(grey)
    assert (g[:, :2] == 0).all() and np.array_equal(g[:, 2], np.arange(256))
    assert np.array_equal(C.hsv_to_rgb_u8(g), grey)
    assert C.rgb_to_hsv_u8(np.zeros((1, 3), np.uint8)).tolist() == [[0, 0, 0]]
    assert C.rgb_to_hsv_u8(np.array([[200, 10, 100]], np.uint8))[0, 0] > 150          # negative h wraps by +180
    assert (C.SDIV[0], C.SDIV[1], C.SDIV[255], C.HDIV[0], C.HDIV[1], C.HDIV[255]) == (0, 1044480, 4096, 0, 122880, 482)


def test_hsv_shift_identity_wrap_and_clip():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    hsv = C.rgb_to_hsv_u8(img)
    assert np.array_equal(C.hsv_shift(img, 0.0, 0.0, 0.0), C.hsv_to_rgb_u8(hsv))       # a shift of 0 leaves H, S, V alone
    base = np.array([[[255, 0, 0]], [[255, 4, 0]], [[255, 0, 8]]], np.uint8)          # H = 0, 0 (rounded from 0.47), 179 (from -0.94)
    assert C.rgb_to_hsv_u8(base)[:, 0, 0].tolist() == [0, 0, 179]

    def h_after(dh):
        out = []
        for px in base:
            h, s, v = C.rgb_to_hsv_u8(px)[0].astype(np.float64)
            out.append(int(np.uint8(np.mod(h + dh, 180.0))))
            want = C.hsv_to_rgb_u8(np.array([[out[-1], s, v]], np.uint8))
            assert np.array_equal(C.hsv_shift(px, dh, 0, 0), want)
        return out
    assert h_after(179.5) == [179, 179, 178]                  # 179.5 -> 179 (truncated); 179 + 179.5 wraps to 178.5
    assert h_after(-0.5) == [179, 179, 178]                   # -0.5 wraps to 179.5
    assert h_after(1.0) == [1, 1, 0]                          # 180 wraps to 0
    # S and V clip at both ends
    c = np.array([[[200, 100, 50]]], np.uint8)
    h, s, v = C.rgb_to_hsv_u8(c)[0, 0]
    assert np.array_equal(C.hsv_shift(c, 0, 300, 0), C.hsv_to_rgb_u8(np.array([[[h, 255, v]]], np.uint8)))
    assert np.array_equal(C.hsv_shift(c, 0, -300, 0), np.full((1, 1, 3), v, np.uint8))          # S = 0: grey v
    assert np.array_equal(C.hsv_shift(c, 0, 0, 300), C.hsv_to_rgb_u8(np.array([[[h, s, 255]]], np.uint8)))
    assert not C.hsv_shift(c, 0, 0, -300).any()
    assert np.array_equal(C.hue(img, 0.25), C.hsv_shift(img, 45.0, 0, 0))


def test_hsv_round_trip_over_the_whole_cube():
    """Every one of the 2^24 colours through RGB -> HSV -> RGB.  Bound 6 grey levels: half a hue unit is worth up to
    255 / 30 / 2 = 4.25 levels, plus the rounding of S and of the output bytes.  Measured maximum: 5."""
    worst = 0
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    for r0 in range(0, 256, 32):
        rgb = np.stack(np.broadcast_arrays(np.arange(r0, r0 + 32, dtype=np.uint8)[:, None, None], g[None], b[None]), -1)
        back = C.hsv_to_rgb_u8(C.rgb_to_hsv_u8(rgb))
        worst = max(worst, int(np.abs(back.astype(np.int16) - rgb.astype(np.int16)).max()))
    print('HSV round trip: maximum error', worst)
    assert worst <= 6


# ---- jitter known answers ---------------------------------------------------------------------------------------------------
def test_brightness_and_contrast_luts():
    at = [0, 1, 127, 255]
    assert C.brightness_lut(0.8)[at].tolist() == [0, 0, 101, 204]              # 0.8, 101.6, 204 truncated
    assert C.brightness_lut(1.2)[at].tolist() == [0, 1, 152, 255]              # 1.2, 152.4, 306 clipped
    # mean 100.  f = 0.8: 1 - 0.8 is 0.19999999999999996 in fp64, so the offset is 19.999999999999996 -> 19 at i = 0; at
    # i = 255 the sum 204 + 19.999999999999996 rounds to 224.0 (half an ulp of 224 is 1.4e-14)
    assert 100.0 * (1 - 0.8) < 20.0
    assert C.contrast_lut(0.8, 100.0)[at].tolist() == [19, 20, 121, 224]
    # f = 1.2: -20.0 and -18.8 clipped, 152.4 - 20 = 132.4, 286 clipped
    assert C.contrast_lut(1.2, 100.0)[at].tolist() == [0, 0, 132, 255]
    img = np.random.default_rng(1).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    assert np.array_equal(C.brightness(img, 1.2), C.brightness_lut(1.2)[img])


def test_contrast_mean_is_the_exact_integer_sum_over_the_pixel_count():
    img = np.random.default_rng(2).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    grey = (9798 * r + 19235 * g + 3735 * b + 16384) >> 15
    assert np.array_equal(C.grey_u8(img), grey) and C.grey_u8(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255
    assert C.contrast_mean(img) == int(grey.sum()) / (37 * 53)
    assert np.array_equal(C.contrast(img, 0.9), C.contrast_lut(0.9, int(grey.sum()) / (37 * 53))[img])


def test_saturation_identity_and_grey():
    img = np.random.default_rng(3).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    assert np.array_equal(C.saturation(img, 1.0), img)
    assert np.array_equal(C.saturation(img, 0.0), np.repeat(C.grey_u8(img)[..., None], 3, -1))
    px = np.array([[[10, 200, 90]]], np.uint8)                                 # grey = (97980 + 3847000 + 336150 + 16384) >> 15 = 131
    assert C.grey_u8(px)[0, 0] == 131
    assert C.saturation(px, 0.5).tolist() == [[[70, 166, 110]]]               # 70.5 and 165.5 round to even, 110.5 too
    assert C.saturation(px, 2.0).tolist() == [[[0, 255, 49]]]                 # saturated at both ends


# ---- keypoints ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['rescale', 'rotate_rescale', 'rescale_rotate'])
def test_keypoints_against_a_scalar_loop(order):
    rot = ('random_rotate', dict(angle_limit=10., p=0.6))
    rs = ('random_rescale', dict(scale_limit=(0.8, 1.25), p=0.6))
    flip = ('horizontal_flip', dict(p=0.5))
    p = _pipe([flip] + dict(rescale=[rs], rotate_rescale=[rot, rs], rescale_rotate=[rs, rot])[order])
    oh, ow = SIZE
    rng = np.random.default_rng(4)
    n = 40
    desc = np.stack([np.zeros(n), rng.integers(1, 300, n), rng.integers(1, 300, n)], 1).astype(np.int64)
    kp = rng.uniform(-5, 300, (n, 9, 2))
    prm = p.draw(n, (9, 0, 0, 2))
    got = p.keypoints(kp, desc, prm)
    assert got.dtype == np.float32 and got.shape == (n, 9, 2)
    both = 0
    for i in range(n):
        mats = {'random_rotate': [R.rotation_matrix(prm['angle'][i], oh, ow)] if prm['rot'][i] else [],
                'random_rescale': [C.rescale_matrix(prm['scale'][i], oh, ow)] if prm['rescale'][i] else []}
        warps = sum((mats[t] for t in p.warp_order), [])
        both += len(warps) == 2
        ref = C.keypoints(kp[i], desc[i, 1], desc[i, 2], oh, ow, bool(prm['flip'][i]), warps, SIZE)
        assert np.array_equal(got[i], ref), (i, order)
    assert order == 'rescale' or both > 3
    # rescale about the centre: the centre stays, a corner moves by the scale
    M = C.rescale_matrix(0.8, oh, ow)
    assert np.allclose(M @ [ow / 2, oh / 2, 1], [ow / 2, oh / 2]) and np.allclose(M @ [0, 0, 1], [0.1 * ow, 0.1 * oh])
