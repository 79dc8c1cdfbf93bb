"""CPU: the Objectron dataset and the compiled augmentation pipeline (dataloaders/objectron.py) on a tiny dataset written
to tmp_path -- annotation parsing, category filtering and the class mapping of objectron_main.py:14-49, the crop of
:98-137 against oracle.crop_resize.objectron_crop, the default config's pipelines, the per-(seed, epoch, rank, batch) draws,
the kernel records and the float64 keypoint arithmetic against tests/augment_ref.py; and that restatement's own checks."""
import json
import os

import numpy as np
import pytest
import torch

import augment_ref as R

CLASSES = ('bike', 'book', 'bottle', 'cereal_box', 'camera', 'chair', 'cup', 'laptop', 'shoe')


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return R.write_dataset(str(tmp_path_factory.mktemp('objectron')), seed=3)


def _cfg(train=None, test=None, norm=R.NORMALIZATION, root='synthetic', **data):
    from torchdet3d.utils import AttrDict
    tr, te = R.default_pipelines((224, 224), norm)
    d = dict(root=root, resize=(224, 224), train_batch_size=4, val_batch_size=3, num_workers=0, category_list='all',
             normalization=R.NORMALIZATION)
    d.update(data)
    return AttrDict(dict(data=d, utils=dict(random_seeds=5), model=dict(num_classes=9),
                         train_data_pipeline=train or tr, test_data_pipeline=test or te))


def test_annotations_filtering_and_class_mapping(root):
    from torchdet3d.dataloaders import Objectron
    ann = json.load(open(os.path.join(root, 'annotations', 'objectron_train.json')))
    ds = Objectron(root, mode='train')
    assert len(ds) == len(ann['annotations']) and ds.num_classes == 9
    for i, a in enumerate(ann['annotations']):
        assert ds.category(i) == a['category_id'] - 1
    keep = sorted({CLASSES[a['category_id'] - 1] for a in ann['annotations']})[:2]
    df = Objectron(root, mode='val', category_list=keep)
    tann = json.load(open(os.path.join(root, 'annotations', 'objectron_test.json')))['annotations']
    sel = [a for a in tann if CLASSES[a['category_id'] - 1] in keep]
    assert len(df) == len(sel) and df.num_classes == 2
    for i, a in enumerate(sel):
        cat_id = a['category_id'] - 1
        assert df.category(i) == min(range(2), key=lambda x: abs(x - cat_id))          # objectron_main.py:56-57
        assert df.annotations[i] is not None and df.images[a['image_id']]['id'] == a['image_id']
    with pytest.raises(RuntimeError):
        Objectron(root, mode='holdout')


def test_items_are_the_oracle_crops(root):
    from PIL import Image
    from oracle.crop_resize import objectron_crop
    from torchdet3d.dataloaders import Objectron
    ds = Objectron(root, mode='test')
    exts = set()
    for i in range(len(ds)):
        frame, crop, kp, cat, cords = ds[i]
        a = ds.annotations[i]
        name = ds.images[a['image_id']]['file_name']
        exts.add(name.rsplit('.', 1)[1])
        ref_frame = np.asarray(Image.open(os.path.join(root, name)).convert('RGB'))
        assert np.array_equal(frame, ref_frame) and frame.dtype == np.uint8
        rkp, rcrop, rcords = objectron_crop(ref_frame, np.asarray(a['keypoints'], np.float64).reshape(9, 2))
        assert cords == rcords and np.array_equal(crop, rcrop) and np.array_equal(kp, rkp)
        assert cat == a['category_id'] - 1
        c2, k2, cat2 = Objectron(root, mode='val')[i]
        assert np.array_equal(c2, crop) and np.array_equal(k2, kp) and cat2 == cat
    assert exts == {'png', 'jpg'}


def test_collate_packs_crops_with_a_descriptor_table(root):
    from torchdet3d.dataloaders import Objectron, collate_crops
    ds = Objectron(root, mode='train')
    items = [ds[i] for i in range(5)]
    packed, desc, kp, cats = collate_crops(items)
    assert packed.dtype == torch.uint8 and desc.dtype == torch.int64 and kp.dtype == torch.float64 and cats.dtype == torch.int64
    for (c, k, cat), (o, h, w), kk, cc in zip(items, desc.tolist(), kp, cats):
        assert (h, w) == c.shape[:2]
        assert np.array_equal(packed[o:o + h * w * 3].numpy().reshape(h, w, 3), c)
        assert np.array_equal(kk.numpy(), k) and int(cc) == cat


def test_default_pipelines_compile():
    from torchdet3d.builders import build_augmentations
    train, test = build_augmentations(_cfg())
    assert train.size == test.size == (224, 224) and train.img_shape == (224, 224)
    assert (train.p_flip, train.p_lut, train.p_rot) == (0.4, 0.3, 0.4)
    assert train.blim == train.clim == (-0.2, 0.2) and train.alim == (-10.0, 10.0)
    assert not train.swap and not test.swap and not test.is_random and train.is_random
    tr, _ = R.default_pipelines()
    bgr, _ = build_augmentations(_cfg(train=tr[1:]))          # no convert_color: the model sees cv.imread's BGR
    assert bgr.swap
    h, w = build_augmentations(_cfg(train=[('resize', dict(height=128, width=160))] + tr[5:]))[0].size
    assert (h, w) == (128, 160)


def test_unsupported_transforms_and_normalisation_mismatch():
    from torchdet3d.builders import build_augmentations
    tr, te = R.default_pipelines()
    with pytest.raises(NotImplementedError, match='blur'):
        build_augmentations(_cfg(train=tr[:4] + [('blur', dict(blur_limit=5, p=0.3))] + tr[4:]))
    with pytest.raises(NotImplementedError, match='one_of'):
        build_augmentations(_cfg(test=te[:2] + [('one_of', dict(p=1, transforms=[]))] + te[2:]))
    with pytest.raises(ValueError, match='normalization'):
        build_augmentations(_cfg(train=tr[:5] + [('normalize', dict(mean=[0.5] * 3, std=[0.25] * 3))] + tr[6:]))
    with pytest.raises(NotImplementedError, match='after random_rotate'):
        build_augmentations(_cfg(train=[tr[1], tr[4], tr[2]] + tr[5:]))


def test_draws_are_deterministic_per_seed_epoch_rank_batch():
    from torchdet3d.builders import build_augmentations
    train, _ = build_augmentations(_cfg())
    a = train.draw(64, (5, 0, 0, 0))
    b = build_augmentations(_cfg())[0].draw(64, (5, 0, 0, 0))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for key in ((6, 0, 0, 0), (5, 1, 0, 0), (5, 0, 1, 0), (5, 0, 0, 1)):
        c = train.draw(64, key)
        assert not np.array_equal(a['angle'], c['angle']) and not np.array_equal(a['alpha'], c['alpha'])
    assert 10 < a['flip'].sum() < 45 and 5 < a['lut'].sum() < 40 and 10 < a['rot'].sum() < 45
    assert np.abs(a['angle']).max() <= 10 and np.abs(a['alpha'] - 1).max() <= 0.2 and np.abs(a['beta']).max() <= 0.2


def test_records_match_the_kernel_abi_and_the_restatement():
    from torchdet3d.builders import build_augmentations
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    train, _ = build_augmentations(_cfg())
    assert AUG_SAMPLE_DTYPE.itemsize == 80 and AUG_SAMPLE_DTYPE.fields['m'][1] == 32
    prm = train.draw(32, (5, 2, 0, 7))
    desc = np.stack([np.arange(32) * 1000, 100 + np.arange(32), 300 - np.arange(32)], 1).astype(np.int64)
    rec = train.records(desc, prm)
    for i in range(32):
        assert (rec['offset'][i], rec['h'][i], rec['w'][i]) == tuple(desc[i])
        assert rec['flags'][i] == (1 if prm['flip'][i] else 0) | (2 if prm['lut'][i] else 0) | (4 if prm['rot'][i] else 0)
        if prm['lut'][i]:
            lut = np.clip(np.arange(256, dtype=np.float32) * rec['alpha'][i] + rec['beta255'][i], 0, 255).astype(np.uint8)
            assert np.array_equal(lut, R.lut_u8(prm['alpha'][i], prm['beta'][i]))
        if prm['rot'][i]:
            assert np.array_equal(rec['m'][i], R.invert_affine(R.rotation_matrix(prm['angle'][i], 224, 224)).reshape(-1))


def test_keypoint_transforms_against_the_float64_restatement():
    from torchdet3d.builders import build_augmentations
    tr, _ = R.default_pipelines((128, 160))
    pipe = build_augmentations(_cfg(train=tr, resize=(128, 160)))[0]
    rng = np.random.default_rng(1)
    B = 40
    desc = np.stack([np.zeros(B), rng.integers(20, 500, B), rng.integers(20, 500, B)], 1).astype(np.int64)
    kp = rng.uniform(0, 1, (B, 9, 2)) * desc[:, None, [2, 1]]
    prm = pipe.draw(B, (1, 2, 3, 4))
    got = pipe.keypoints(kp, desc, prm)
    assert got.dtype == np.float32 and got.shape == (B, 9, 2)
    for i in range(B):
        ref = R.keypoints(kp[i], desc[i, 1], desc[i, 2], 128, 160, bool(prm['flip'][i]),
                          float(prm['angle'][i]) if prm['rot'][i] else None)
        assert np.array_equal(got[i], ref), i


def test_build_loader_serves_objectron_for_a_data_root(root):
    from torchdet3d.builders import build_loader
    cfg = _cfg(root=root)
    train, val, test = build_loader(cfg)
    assert len(train) == len(train.dataset) // 4 and len(val) == -(-len(val.dataset) // 3) and len(test) == len(test.dataset)
    train.sampler.set_epoch(3)
    assert train.sampler.epoch == 3 and train.seed == 5 and train.pipeline.is_random and not val.pipeline.is_random
    assert test.dataset.mode == 'test'
    with pytest.raises(NotImplementedError):
        tr, te = R.default_pipelines()
        build_loader(_cfg(root=root, train=tr[:2] + [('rgb_shift', dict(p=0.3))] + tr[2:]))


def test_restated_lut_and_flip():
    assert np.array_equal(R.lut_u8(1.0, 0.0), np.arange(256))
    lut = R.lut_u8(1.15, -0.1)
    assert lut.dtype == np.uint8 and lut[0] == 0 and lut[255] == 255
    assert lut[100] == np.uint8(np.float32(np.float32(100) * np.float32(1.15)) + np.float32(-0.1 * 255))
    img = np.arange(2 * 5 * 3, dtype=np.uint8).reshape(2, 5, 3)
    out = R.augment(img, 2, 5, flip=True)
    assert np.array_equal(out, img[:, ::-1])


@pytest.mark.parametrize('angle', [10.0, -10.0, 3.7, 1e-3])
def test_restated_warp_against_textbook_bilinear(angle):
    """The fixed-point warp within 1 grey level of the fp64 bilinear on a smooth image (away from the source border,
    where the zero border makes a step), and within 9 on uniform noise: a coordinate is rounded to 1/32 pixel, i.e. off
    by at most 1/64 pixel per axis, worth at most 255 / 64 per axis on noise, plus the final rounding."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:224, 0:224]
    smooth = np.clip(np.stack([127 + 100 * np.sin(xx / 19. + c) * np.cos(yy / 29. - c) for c in range(3)], -1), 0, 255)
    smooth = smooth.astype(np.uint8)
    noise = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    M = R.rotation_matrix(angle, 224, 224)
    mi = np.linalg.inv(np.vstack([M, [0, 0, 1]]))
    sx, sy = mi[0, 0] * xx + mi[0, 1] * yy + mi[0, 2], mi[1, 0] * xx + mi[1, 1] * yy + mi[1, 2]
    inside = (sx >= 1) & (sx <= 222) & (sy >= 1) & (sy <= 222)
    d = np.abs(R.warp_affine_u8(smooth, M).astype(np.float64) - R.warp_affine_float(smooth, M))
    assert d[inside].max() < 1.0
    d = np.abs(R.warp_affine_u8(noise, M).astype(np.float64) - R.warp_affine_float(noise, M))
    assert d.max() < 9.0
    assert np.array_equal(R.warp_affine_u8(noise, R.rotation_matrix(0.0, 224, 224)), noise)
