"""GPU: `t3d_augment_chain_crops_u8` / `t3d_augment_chain_resized_u8` (csrc/augment_chain.hip) bit-exact against the numpy
restatement (tests/augment_chain_ref.py): every colour op alone and chained on a colour lattice that walks every branch of
the HSV pair, small and odd outputs, tiny crops, mixed batches, all 24 jitter orders (the contrast mean is checked through
the output), both warp orders, the arena entry point against the crops entry point, bad records and arguments; and the
loader with the three transforms, cached against uncached against the restatement, beside the default loader."""
import itertools

import numpy as np
import pytest
import torch

import augment_chain_ref as C
import augment_ref as R

pytestmark = pytest.mark.gpu

KIND = dict(lut=1, hsv=2, brightness=3, contrast=4, saturation=5, hue=6)
JITTER = ('brightness', 'contrast', 'saturation', 'hue')


def _records(specs, oh, ow):
    """specs: dicts with crop, flip, swap, lut (alpha, beta: the BASE record's LUT), ops [(name, *p)], warps [forward 2x3]
    -> (packed crops, base records, chain records)."""
    from torchdet3d.dataloaders.objectron import AUG_CHAIN_DTYPE, AUG_SAMPLE_DTYPE
    B = len(specs)
    rec, ext = np.zeros(B, AUG_SAMPLE_DTYPE), np.zeros(B, AUG_CHAIN_DTYPE)
    parts, off = [], 0
    for i, s in enumerate(specs):
        c = s['crop']
        rec['offset'][i], rec['h'][i], rec['w'][i] = off, c.shape[0], c.shape[1]
        parts.append(c.reshape(-1))
        off += c.size
        fl = (1 if s.get('flip') else 0) | (8 if s.get('swap') else 0)
        rec['alpha'][i] = 1.0
        if s.get('lut'):
            fl |= 2
            rec['alpha'][i], rec['beta255'][i] = np.float32(s['lut'][0]), np.float32(s['lut'][1] * 255)
        warps = s.get('warps', ())
        if warps:
            fl |= 4
            rec['m'][i] = R.invert_affine(warps[0]).reshape(-1)
        if len(warps) > 1:
            ext['flags'][i] = 1
            ext['m2'][i] = R.invert_affine(warps[1]).reshape(-1)
        rec['flags'][i] = fl
        ops = s.get('ops', ())
        ext['n_ops'][i] = len(ops)
        for k, (name, *p) in enumerate(ops):
            ext['kind'][i, k] = KIND[name]
            if name == 'lut':
                p = [np.float32(p[0]), np.float32(p[1] * 255)]
            ext['p'][i, k, :len(p)] = p
    return np.concatenate(parts), rec, ext


def _launch(name, src, rec, ext, oh, ow, stages=None, scratch_bytes=None):
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.objectron import chain_scratch_bytes, chain_stages
    B = len(rec)
    stages = chain_stages(rec, ext) if stages is None else stages
    srcd = src if torch.is_tensor(src) else torch.from_numpy(src).cuda()
    recd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    extd = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    nb = chain_scratch_bytes(B, oh, ow, stages) if scratch_bytes is None else scratch_bytes
    scratch = torch.full((max(nb, 8),), 0xA5, dtype=torch.uint8, device='cuda')          # (stale sums must not leak in)
    out = torch.full((B, oh, ow, 3), 77, dtype=torch.uint8, device='cuda')
    N.call(name, N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch), nb, N.ptr(out), B, oh, ow, stages,
           N.stream())
    return out.cpu().numpy()


def _ref(s, oh, ow):
    ops = ([('lut',) + tuple(s['lut'])] if s.get('lut') else []) + list(s.get('ops', ()))
    return C.chain(s['crop'], oh, ow, s.get('flip', False), ops, s.get('warps', ()), s.get('swap', False))


def _check(specs, oh, ow, arena=False):
    """The crops entry point against the restatement; arena=True: also the arena entry point on the same records."""
    src, rec, ext = _records(specs, oh, ow)
    got = _launch('t3d_augment_chain_crops_u8', src, rec, ext, oh, ow)
    for i, s in enumerate(specs):
        ref = _ref(s, oh, ow)
        assert np.array_equal(got[i], ref), (i, s['crop'].shape, {k: v for k, v in s.items() if k != 'crop'},
                                             int(np.abs(got[i].astype(int) - ref.astype(int)).max()))
    if arena:
        from torchdet3d import _native as N
        from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
        B = len(specs)
        plain = np.zeros(B, AUG_SAMPLE_DTYPE)
        plain['offset'], plain['h'], plain['w'] = rec['offset'], rec['h'], rec['w']
        srcd, pd = torch.from_numpy(src).cuda(), torch.from_numpy(plain.view(np.uint8).copy()).cuda()
        resized = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device='cuda')
        N.call('t3d_augment_crops_u8', N.ptr(srcd), srcd.numel(), N.ptr(pd), N.ptr(resized), B, oh, ow, N.stream())
        pad = 5                                                          # slots at odd addresses, walked backwards
        arena_t = torch.zeros(pad + B * oh * ow * 3, dtype=torch.uint8, device='cuda')
        arena_t[pad:] = resized.flip(0).reshape(-1)
        ra = rec.copy()
        ra['offset'], ra['h'], ra['w'] = pad + (B - 1 - np.arange(B)) * oh * ow * 3, oh, ow
        got_a = _launch('t3d_augment_chain_resized_u8', arena_t, ra, ext, oh, ow)
        assert np.array_equal(got_a, got), [i for i in range(B) if not np.array_equal(got_a[i], got[i])]
    return got


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(np.stack([127 + 110 * np.sin(xx / 13. + k) * np.cos(yy / 17. - k) for k in range(3)], -1)
                   + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)


def _lattice():
    """64 x 64 pixels: every (r, g, b) of 16 levels a channel, 0 and 255 among them -- v == r, v == g, v == b, all the ties,
    s == 0 and negative h all occur."""
    lv = (np.arange(16) * 17).astype(np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing='ij')
    return np.ascontiguousarray(np.stack([r, g, b], -1).reshape(64, 64, 3))


ALONE = [('hsv', 7.3, -12.5, 9.25), ('hsv', -19.5, 30.0, -20.0), ('hsv', 179.5, 0.0, 0.0), ('hsv', -0.5, 300.0, -300.0),
         ('hsv', 0.0, 0.0, 0.0), ('brightness', 0.8), ('brightness', 1.2), ('contrast', 0.8), ('contrast', 1.2),
         ('saturation', 0.7), ('saturation', 1.3), ('saturation', 0.0), ('hue', 0.13), ('hue', -0.2), ('hue', 0.5),
         ('lut', 1.17, -0.13)]


def test_each_colour_op_alone_and_all_chained_on_the_lattice():
    lat = _lattice()
    specs = [dict(crop=lat, ops=[op]) for op in ALONE]
    specs.append(dict(crop=lat, ops=[('hsv', 7.3, -12.5, 9.25), ('lut', 0.9, 0.1), ('saturation', 1.15), ('brightness', 1.1),
                                     ('hue', -0.07), ('contrast', 0.85)], flip=True))
    specs.append(dict(crop=lat, lut=(1.1, -0.05), ops=[('contrast', 1.2), ('hue', 0.2), ('brightness', 0.9), ('saturation', 0.8),
                                                       ('hsv', -5.0, 10.0, -10.0), ('lut', 1.05, 0.02), ('hsv', 1.0, 1.0, 1.0),
                                                       ('hue', 0.01)], swap=True))          # 8 ops: a full program
    got = _check(specs, 64, 64, arena=True)
    assert np.array_equal(_check([dict(crop=lat)], 64, 64)[0], lat)                     # the resize is the identity here
    assert np.array_equal(got[4], C.hsv_to_rgb_u8(C.rgb_to_hsv_u8(lat)))                  # a zero shift is the round trip


@pytest.mark.parametrize('oh,ow', [(7, 5), (96, 80)])
@pytest.mark.parametrize('B', [1, 5])
def test_small_outputs_tiny_crops_mixed_batches(oh, ow, B):
    """7 x 5: an odd pixel count, a plane that is no multiple of a thread's run; 96 x 80: eight workgroups a sample, so the
    grey sum crosses workgroups."""
    rng = np.random.default_rng(oh * 10 + B)
    everything = dict(flip=True, swap=True, ops=[('lut', 1.1, 0.05), ('hsv', 11.0, -20.0, 15.0), ('saturation', 1.2),
                                                 ('contrast', 0.8), ('hue', 0.1), ('brightness', 1.15)],
                      warps=[R.rotation_matrix(-7.0, oh, ow), C.rescale_matrix(1.25, oh, ow)])
    if B == 1:
        specs = [dict(everything, crop=_smooth(rng, 201, 150))]
    else:
        specs = [dict(crop=_noise(rng, 1, 1), ops=[('contrast', 1.2), ('hue', 0.3)]),
                 dict(crop=_noise(rng, 2, 2), ops=[('hsv', -3.0, 8.0, 2.0)], flip=True),
                 dict(crop=_noise(rng, 37, 53)),                                          # nothing fired ...
                 dict(everything, crop=_noise(rng, 37, 53)),                              # ... next to everything
                 dict(crop=_smooth(rng, 160, 230), ops=[('saturation', 0.9), ('contrast', 1.1)],
                      warps=[C.rescale_matrix(0.8, oh, ow)])]
    got = _check(specs, oh, ow, arena=True)
    if B == 5:
        assert np.array_equal(got[2], R.augment(specs[2]['crop'], oh, ow))                # n_ops 0 == t3d_augment_crops_u8


def test_every_jitter_order_and_the_contrast_mean_through_the_output():
    rng = np.random.default_rng(24)
    oh, ow = 96, 80
    crop = _smooth(rng, 140, 111)
    f = dict(brightness=1.18, contrast=0.82, saturation=1.15, hue=-0.12)
    specs = [dict(crop=crop, flip=bool(i & 1), ops=[(JITTER[k], f[JITTER[k]]) for k in order])
             for i, order in enumerate(itertools.permutations(range(4)))]
    assert len(specs) == 24
    got = _check(specs, oh, ow)
    assert len({g[:, ::-1].tobytes() if i & 1 else g.tobytes() for i, g in enumerate(got)}) > 1       # the order matters
    # the mean is that of the image contrast meets: with a wrong one (the resized image's) the restatement differs
    img = R.resize_linear_u8(crop, (ow, oh))
    pre = C.brightness(img, f['brightness'])
    assert C.contrast_mean(pre) != C.contrast_mean(img)
    assert not np.array_equal(C.contrast_lut(f['contrast'], C.contrast_mean(img))[pre], C.contrast(pre, f['contrast']))


@pytest.mark.parametrize('scale', [0.8, 1.25])
def test_both_warp_orders(scale):
    rng = np.random.default_rng(int(scale * 100))
    oh, ow = 96, 80
    rot, rs = R.rotation_matrix(8.5, oh, ow), C.rescale_matrix(scale, oh, ow)
    colour = [('hsv', 5.0, 5.0, -5.0), ('contrast', 1.1)]
    specs = [dict(crop=_smooth(rng, 150, 170), warps=[rs]),
             dict(crop=_smooth(rng, 99, 240), warps=[rot, rs]),
             dict(crop=_smooth(rng, 99, 240), warps=[rs, rot]),
             dict(crop=_noise(rng, 64, 64), warps=[rot, rs], flip=True, swap=True, ops=colour),
             dict(crop=_noise(rng, 64, 64), warps=[rs, rot], flip=True, swap=True, ops=colour),
             dict(crop=_noise(rng, 30, 20), warps=[C.rescale_matrix(0.0, oh, ow)]),        # singular: D == 0, the zero map
             dict(crop=_noise(rng, 30, 20), warps=[C.rescale_matrix(-0.1, oh, ow), rot])]  # (the reference's default limits)
    got = _check(specs, oh, ow, arena=True)
    assert not np.array_equal(got[1], got[2])                                            # two roundings: the order shows
    # each warp rounds to uint8: the two in a row are not one warp by the product matrix
    both = np.vstack([rs, [0, 0, 1]]) @ np.vstack([rot, [0, 0, 1]])
    assert not np.array_equal(got[1], R.warp_affine_u8(R.resize_linear_u8(specs[1]['crop'], (ow, oh)), both[:2]))


def test_bad_chain_records_give_zeros_and_leave_their_neighbours():
    from torchdet3d import _native as N
    rng = np.random.default_rng(3)
    oh, ow = 13, 17
    ok = dict(ops=[('hsv', 4.0, 4.0, 4.0), ('contrast', 0.9)], warps=[R.rotation_matrix(5.0, oh, ow), C.rescale_matrix(0.9, oh, ow)])
    specs = [dict(ok, crop=_noise(rng, 20 + i, 31 - i), flip=bool(i & 1)) for i in range(12)]
    src, rec, ext = _records(specs, oh, ow)
    good = _launch('t3d_augment_chain_crops_u8', src, rec, ext, oh, ow)
    assert all(g.any() for g in good)
    bad, badrec = ext.copy(), rec.copy()
    bad['n_ops'][0] = 9
    bad['n_ops'][2] = -1
    bad['kind'][3, 0] = 0
    bad['kind'][5, 1] = 7
    bad['flags'][6] = 3
    bad['kind'][8, 0] = 4                                    # a second CONTRAST op
    badrec['flags'][9] &= ~4                                 # a second warp without a first
    badrec['h'][11] = 0                                      # a base record t3d_augment_crops_u8 refuses
    zero = [0, 2, 3, 5, 6, 8, 9, 11]
    out = _launch('t3d_augment_chain_crops_u8', src, badrec, bad, oh, ow, stages=7)
    for j in range(12):
        assert (out[j] == 0).all() if j in zero else np.array_equal(out[j], good[j]), j
    # a record that needs a stage the call does not name is a bad record, whatever else is launched
    for stages, dead in ((6, 'contrast'), (3, 'second warp'), (1, 'warps'), (0, 'all')):
        out = _launch('t3d_augment_chain_crops_u8', src, rec, ext, oh, ow, stages=stages)
        assert not out.any(), dead
    mixed_specs = [dict(crop=specs[0]['crop'], ops=[('hue', 0.1)]), specs[1]]
    ms, mr, me = _records(mixed_specs, oh, ow)
    out = _launch('t3d_augment_chain_crops_u8', ms, mr, me, oh, ow, stages=0)
    assert np.array_equal(out[0], _ref(mixed_specs[0], oh, ow)) and not out[1].any()
    # arguments
    need = 8 * 12 + 2 * ((12 * oh * ow * 3 + 7) // 8 * 8)
    _launch('t3d_augment_chain_crops_u8', src, rec, ext, oh, ow, stages=7, scratch_bytes=need)
    for kw in (dict(stages=7, scratch_bytes=need - 1), dict(stages=8), dict(stages=4), dict(stages=5), dict(stages=-1)):
        with pytest.raises(RuntimeError):
            _launch('t3d_augment_chain_crops_u8', src, rec, ext, oh, ow, **kw)
    srcd, recd = torch.from_numpy(src).cuda(), torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    extd = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    scratch, out = torch.zeros(need + 8, dtype=torch.uint8, device='cuda'), torch.zeros(12, oh, ow, 3, dtype=torch.uint8, device='cuda')
    for name in ('t3d_augment_chain_crops_u8', 't3d_augment_chain_resized_u8'):
        for args in ((N.ptr(srcd), srcd.numel(), N.ptr(recd), None, N.ptr(scratch), need, N.ptr(out), 12, oh, ow, 7),
                     (N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), None, need, N.ptr(out), 12, oh, ow, 7),
                     (N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch) + 4, need, N.ptr(out), 12, oh, ow, 7),
                     (N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch), need, N.ptr(out) + 2, 12, oh, ow, 7),
                     (N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch), need, N.ptr(out), 12, 0, ow, 7),
                     (N.ptr(srcd), 0, N.ptr(recd), N.ptr(extd), N.ptr(scratch), need, N.ptr(out), 12, oh, ow, 7),
                     (N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch), need, N.ptr(out), 65536, oh, ow, 7)):
            with pytest.raises(RuntimeError):
                N.call(name, *args, N.stream())
    N.call('t3d_augment_chain_crops_u8', N.ptr(srcd), srcd.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch), need, N.ptr(out), 0,
           oh, ow, 7, N.stream())                                                         # an empty batch is no error


# ---- the loader ----------------------------------------------------------------------------------------------------------------
SIZE = (96, 80)


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return R.write_dataset(str(tmp_path_factory.mktemp('objectron')), seed=6, n_train=12, n_test=6)


def _cfg(root, chained, **data):
    from torchdet3d.utils import AttrDict
    tr, te = R.default_pipelines(SIZE)
    if chained:
        tr = tr[:2] + [('hue_saturation_value', dict(p=0.6)), tr[2], ('color_jitter', dict(p=0.7)), tr[3],
                       ('random_rescale', dict(scale_limit=(0.8, 1.25), p=0.6)), tr[4]] + tr[5:]
        te = te[:2] + [('color_jitter', dict(p=1.0))] + te[2:]
    d = dict(root=root, resize=SIZE, train_batch_size=5, val_batch_size=4, num_workers=0, category_list='all',
             normalization=R.NORMALIZATION)
    d.update(data)
    return AttrDict(dict(data=d, utils=dict(random_seeds=5), model=dict(num_classes=9), train_data_pipeline=tr,
                         test_data_pipeline=te))


def _batches(loader, epoch):
    if hasattr(loader.sampler, 'set_epoch'):
        loader.sampler.set_epoch(epoch)
    return [tuple(t.cpu().numpy().copy() for t in b) for b in loader], [list(ix) for ix in loader.loader.batch_sampler]


def _spec_of(pipe, prm, i, crop):
    """The restatement's arguments for sample i of a draw, in the config's order."""
    oh, ow = pipe.size
    ops = []
    for t in pipe.colour_order:
        if t == 'random_brightness_contrast' and prm['lut'][i]:
            ops.append(('lut', prm['alpha'][i], prm['beta'][i]))
        if t == 'hue_saturation_value' and prm['hsv'][i]:
            ops.append(('hsv', prm['dh'][i], prm['ds'][i], prm['dv'][i]))
        if t == 'color_jitter' and prm['jit'][i]:
            ops += [(JITTER[k], prm[('jb', 'jc', 'js', 'jh')[k]][i]) for k in prm['order'][i]]
    warps = []
    for t in pipe.warp_order:
        if t == 'random_rotate' and prm['rot'][i]:
            warps.append(R.rotation_matrix(prm['angle'][i], oh, ow))
        if t == 'random_rescale' and pipe.chained and prm['rescale'][i]:
            warps.append(C.rescale_matrix(prm['scale'][i], oh, ow))
    return dict(crop=crop, flip=bool(prm['flip'][i]), swap=pipe.swap, ops=ops, warps=warps)


@pytest.mark.parametrize('chained', [True, False])
def test_loader_cached_equals_uncached_equals_the_restatement(root, chained):
    """chained: the three new transforms in both loader modes over two epochs -- images, keypoints, classes.  Not chained:
    the default pipeline serves what it served before (tests/augment_ref.py's augment and keypoints)."""
    from torchdet3d.builders import build_loader
    plain = build_loader(_cfg(root, chained))
    cached = build_loader(_cfg(root, chained, cache='device'))
    fired = set()
    for which in (0, 1):                                     # train and val
        pipe = plain[which].pipeline
        assert pipe.chained == chained
        for epoch in (0, 1):
            ref, order = _batches(plain[which], epoch)
            got, _ = _batches(cached[which], epoch)
            assert len(ref) == len(got) > 0
            for b, (x, y, ix) in enumerate(zip(got, ref, order)):
                assert all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(x, y)), (which, epoch, b)
                if epoch == 1 and which == 1:
                    continue                                 # (the restatement once per loader and train epoch)
                prm = pipe.draw(len(ix), (5, epoch, 0, b))
                for i, idx in enumerate(ix):
                    crop, kp, cat = plain[which].dataset.host[idx]
                    s = _spec_of(pipe, prm, i, crop)
                    if chained:
                        img = C.chain(crop, *SIZE, s['flip'], s['ops'], s['warps'], s['swap'])
                    else:
                        img = R.augment(crop, *SIZE, s['flip'], prm['alpha'][i] if prm['lut'][i] else 1.0,
                                        prm['beta'][i] if prm['lut'][i] else 0.0, prm['angle'][i] if prm['rot'][i] else None)
                        assert np.array_equal(y[1][i], R.keypoints(kp, crop.shape[0], crop.shape[1], *SIZE, s['flip'],
                                                                   prm['angle'][i] if prm['rot'][i] else None, SIZE))
                    assert np.array_equal(y[0][i], img), (which, epoch, b, i, s['ops'])
                    assert np.array_equal(y[1][i], C.keypoints(kp, crop.shape[0], crop.shape[1], *SIZE, s['flip'], s['warps'], SIZE))
                    assert y[2][i] == cat
                    fired.add((len(s['ops']) > 0, len(s['warps'])))
    assert {w for _, w in fired} == ({0, 1, 2} if chained else {0, 1}) and {o for o, _ in fired} == {False, True}
    item = plain[0].dataset[3]                               # a batch of one through the same path
    assert item[0].shape == SIZE + (3,) and item[0].is_cuda
