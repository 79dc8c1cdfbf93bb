"""CPU: the host half of the detection loader -- the record layout against include/t3d.h, the draws, the box arithmetic of
`DetectionAugmentPipeline` against the step-by-step restatement (tests/detect_augment_ref.py), the invariants of every drawn
crop, the coverage of every branch by the chosen seed, `ObjectronFrames`' filters, and what the compiler refuses."""
import json
import os
import re

import numpy as np
import pytest
from PIL import Image

import detect_augment_ref as D
from conftest import ROOT

TRAIN = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion', brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18),
    dict(type='Albu', transforms=[dict(type='RandomRotate90and270', p=0.5)],
         bbox_params=dict(type='BboxParams', format='pascal_voc', label_fields=['gt_labels'], min_visibility=0.0,
                          filter_lost_elements=True),
         update_pad_shape=False, skip_img_without_anno=True),
    dict(type='Expand', ratio_range=(1, 3)),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.1),
    dict(type='Resize', img_scale=(300, 300), keep_ratio=False),
    dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]
TEST = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(300, 300), flip=False,
         transforms=[dict(type='Resize', keep_ratio=False), dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
                     dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]),
]
SEED, NBATCH, BATCH = 0, 24, 8          # 192 drawn samples; the seed is chosen so that they reach every branch (asserted below)


def _pipe(steps=TRAIN, size=(300, 300)):
    from torchdet3d.dataloaders import DetectionAugmentPipeline
    return DetectionAugmentPipeline(steps, size)


def _scene(rng, n):
    """n frames' sizes (40x30 ... 97x64, either orientation) with 1-4 boxes each; four in ten hold ONE object that nearly fills
    the frame -- the only scenes in which the crop modes .7 and .9 can return (every box needs that IoU with the patch)."""
    desc, boxes, labels, off = np.zeros((n, 3), np.int64), [], [], 0
    for i in range(n):
        h, w = int(rng.integers(30, 65)), int(rng.integers(40, 98))
        if rng.random() < .3:
            h, w = w, h
        desc[i] = off, h, w
        off += h * w * 3
        k = int(rng.integers(1, 5))
        x0, y0 = rng.uniform(0, w * .6, k), rng.uniform(0, h * .6, k)
        bw, bh = rng.uniform(3, w * .4, k), rng.uniform(3, h * .4, k)
        if rng.random() < .4:
            k = 1
            x0, y0 = rng.uniform(0, w * .03, 1), rng.uniform(0, h * .03, 1)
            bw, bh = w * rng.uniform(.97, 1, 1) - x0, h * rng.uniform(.97, 1, 1) - y0
        boxes.append(np.stack([x0, y0, x0 + bw, y0 + bh], 1).astype(np.float32))
        labels.append(rng.integers(0, 9, k).astype(np.int32))
    return desc, boxes, labels


@pytest.fixture(scope='module')
def drawn():
    """192 samples through draw / boxes / records, each beside the restatement's step-by-step result."""
    pipe, rng, rows = _pipe(), np.random.default_rng(11), []
    for batch in range(NBATCH):
        key = (SEED, 0, 0, batch)
        desc, boxes, labels = _scene(rng, BATCH)
        prm = pipe.draw(BATCH, key)
        got_b, got_l = pipe.boxes(boxes, labels, desc, prm)
        rec = pipe.records(desc, prm)
        for i in range(BATCH):
            frame = np.zeros((int(desc[i, 1]), int(desc[i, 2]), 3), np.uint8)
            crop_rng = np.random.default_rng(list(key) + [D.CROP_TAG, i])
            _, ref_b, ref_l, info = D.sample(frame, boxes[i], labels[i], D.params_of(prm, i), 300, 300, crop_rng, 0.1)
            rows.append(dict(got_b=got_b[i], got_l=got_l[i], ref_b=ref_b, ref_l=ref_l, info=info, rec=rec[i],
                             mode=prm['mode'][i], geom=prm['geom'][i], canvas=prm['canvas'][i],
                             prm={k: v[i] for k, v in prm.items() if k not in ('key',)}, hw=(int(desc[i, 1]), int(desc[i, 2]))))
    return rows


def test_record_dtype_matches_the_header():
    """(DET_SAMPLE_DTYPE against the compiler's layout of t3d_det_sample, member by member: tests/test_abi.py.)"""
    from torchdet3d.dataloaders.detection import DET_SAMPLE_DTYPE
    src = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    assert DET_SAMPLE_DTYPE.itemsize == 80
    flags = dict(re.findall(r'(T3D_DET_\w+) = (\d+)', src))
    from torchdet3d.dataloaders import detection as M
    assert {k: int(v) for k, v in flags.items()} == dict(
        T3D_DET_FLIP=M.DET_FLIP, T3D_DET_BRIGHTNESS=M.DET_BRIGHTNESS, T3D_DET_CONTRAST=M.DET_CONTRAST,
        T3D_DET_CONTRAST_LAST=M.DET_CONTRAST_LAST, T3D_DET_HSV=M.DET_HSV, T3D_DET_SATURATION=M.DET_SATURATION, T3D_DET_HUE=M.DET_HUE)


def test_draws_are_reproducible_per_key_and_differ_across_batch_epoch_rank():
    pipe = _pipe()

    def flat(key):
        prm = pipe.draw(16, key)
        return np.concatenate([np.asarray(prm[k], np.float64).reshape(-1) for k in sorted(prm) if k != 'key'])
    base = flat((5, 0, 0, 0))
    assert np.array_equal(base, flat((5, 0, 0, 0)))
    for other in ((5, 0, 0, 1), (5, 1, 0, 0), (5, 0, 1, 0), (6, 0, 0, 0)):
        assert not np.array_equal(base, flat(other)), other
    # the crop search is keyed too: the same key gives the same patch, another batch another one
    desc, boxes, labels = _scene(np.random.default_rng(0), 16)
    geoms = []
    for key in ((5, 0, 0, 0), (5, 0, 0, 0), (5, 0, 0, 1)):
        prm = pipe.draw(16, key)
        pipe.boxes(boxes, labels, desc, prm)
        geoms.append(prm['geom'])
    assert np.array_equal(geoms[0], geoms[1]) and not np.array_equal(geoms[0], geoms[2])


def test_boxes_equal_the_step_by_step_restatement(drawn):
    assert len(drawn) >= 100
    for r in drawn:
        assert r['got_b'].dtype == np.float32 and r['got_b'].shape == r['ref_b'].shape
        assert np.array_equal(r['got_b'], r['ref_b'])
        assert np.array_equal(r['got_l'], r['ref_l'])
        # and the records carry the geometry the restatement chose
        rec, info = r['rec'], r['info']
        H, W = info['canvas']
        patch = info['patch'] if info['patch'] is not None else (0, 0, W, H)
        assert (rec['cx0'], rec['cy0'], rec['cx1'], rec['cy1']) == tuple(patch)
        assert rec['turns'] == r['prm']['turns']
        # ... and so do the package's own prm['mode'] / prm['geom'] / prm['canvas']
        assert r['mode'] == info['mode'] and tuple(r['geom'][3:]) == tuple(patch) and tuple(r['canvas']) == (H, W)
        assert r['geom'][0] == r['prm']['turns']


def test_every_drawn_crop_keeps_mmdets_invariants(drawn):
    for r in drawn:
        info = r['info']
        assert len(r['got_b']) >= 1
        b = r['got_b']
        assert (b >= 0).all() and (b[:, [0, 2]] <= 300).all() and (b[:, [1, 3]] <= 300).all()
        if info['patch'] is None:
            assert info['mode'] == 1
            continue
        x0, y0, x1, y1 = info['patch']
        # mmdet tests new_h / new_w of the REAL-valued size it drew, before the corners are truncated to integers: that ratio
        # is in [.5, 2], and each side of the integer patch is within one pixel of the drawn one
        new_w, new_h = info['drawn']
        assert 0.5 <= new_h / new_w <= 2
        assert abs((x1 - x0) - new_w) <= 1 and abs((y1 - y0) - new_h) <= 1
        before, mask = info['before'], info['mask']
        assert mask.any()
        c = (before[:, :2] + before[:, 2:]) / 2
        inside = (c[:, 0] > x0) & (c[:, 1] > y0) & (c[:, 0] < x1) & (c[:, 1] < y1)
        assert np.array_equal(inside, mask)
        assert (D.iou_with_patch((x0, y0, x1, y1), before) >= info['mode']).all()


def test_the_seed_reaches_every_branch(drawn):
    modes = {r['info']['mode'] for r in drawn}
    assert modes == {1, .1, .3, .5, .7, .9, 0}
    assert {bool(r['prm']['first']) for r in drawn if r['prm']['contrast']} == {True, False}
    assert {int(r['prm']['turns']) for r in drawn} == {0, 1, 3}
    assert {bool(r['prm']['expand']) for r in drawn} == {True, False}
    assert {bool(r['prm']['flip']) for r in drawn} == {True, False}
    for k in ('bright', 'contrast', 'sat_on', 'hue_on'):
        assert {bool(r['prm'][k]) for r in drawn} == {True, False}, k
    assert len({tuple(r['prm']['perm']) for r in drawn}) == 6


def _write_dataset(root, images, annotations, name='objectron_train.json'):
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    rng = np.random.default_rng(0)
    imgs = []
    for k, (iid, h, w) in enumerate(images):
        fn = f'images/{iid:04d}.png'
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, fn))
        imgs.append(dict(id=iid, file_name=fn, width=w, height=h))
    anns = [dict(id=k, image_id=iid, category_id=cat, bbox=list(bbox), iscrowd=crowd, area=bbox[2] * bbox[3])
            for k, (iid, cat, bbox, crowd) in enumerate(annotations)]
    with open(os.path.join(root, 'annotations', name), 'w') as f:
        json.dump(dict(images=imgs, annotations=anns, categories=[]), f)


def test_objectron_frames_filters(tmp_path):
    from torchdet3d.dataloaders import ObjectronFrames
    from torchdet3d.utils import OBJECTRON_CLASSES
    root = str(tmp_path)
    images = [(7, 30, 40), (3, 24, 32), (9, 20, 20), (4, 16, 40), (5, 30, 30), (6, 30, 30)]
    anns = [(7, 1, (2, 3, 10, 12), 0), (7, 3, (5, 5, 20.5, 10), 0), (7, 2, (1, 1, 8, 8), 1),      # image 7: two boxes + a crowd
            (3, 2, (4, 4, 0.5, 9), 0), (3, 2, (4, 4, 9, 0.9), 0), (3, 5, (1, 2, 3, 4), 0),        # image 3: two sub-pixel boxes + one
            (9, 2, (1, 1, 5, 5), 1),                                                              # image 9: only a crowd -> empty
            (4, 1, (1, 1, 5, 5), 0),                                                              # image 4: min(h, w) = 16 < 17
            (5, 4, (1, 1, 5, 5), 0)]                                                              # image 5: one box; image 6: none
    _write_dataset(root, images, anns)
    _write_dataset(root, images, anns, 'objectron_test.json')
    ds = ObjectronFrames(root, 'train')
    assert ds.image_ids == [7, 3, 5]                    # the json's order, not the ids'
    frame, boxes, labels = ds[0]
    assert frame.dtype == np.uint8 and frame.shape == (30, 40, 3)
    with Image.open(os.path.join(root, 'images/0007.png')) as im:
        assert np.array_equal(frame, np.asarray(im))
    assert boxes.dtype == np.float32 and labels.dtype == np.int32
    assert np.array_equal(boxes, np.array([[2, 3, 12, 15], [5, 5, 25.5, 15]], np.float32)) and list(labels) == [0, 2]
    assert np.array_equal(ds[1][1], np.array([[1, 2, 4, 6]], np.float32)) and list(ds[1][2]) == [4]
    # min_size is a setting; the val / test mode keeps every image, empty ones too
    assert ObjectronFrames(root, 'train', min_size=16).image_ids == [7, 3, 4, 5]
    dv = ObjectronFrames(root, 'val')
    assert dv.image_ids == [7, 3, 9, 4, 5, 6] and dv[2][1].shape == (0, 4) and dv[5][2].shape == (0,)
    # the category filter: names of OBJECTRON_CLASSES; the label stays category_id - 1
    keep = [OBJECTRON_CLASSES[0], OBJECTRON_CLASSES[4]]
    dc = ObjectronFrames(root, 'train', category_list=keep)
    assert dc.image_ids == [7, 3] and list(dc[0][2]) == [0] and list(dc[1][2]) == [4]
    with pytest.raises(RuntimeError):
        ObjectronFrames(root, 'nope')


def test_collate_frames_packs_frames_boxes_and_counts():
    from torchdet3d.dataloaders import collate_frames
    rng = np.random.default_rng(0)
    items = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.random((n, 4)).astype(np.float32), np.arange(n, dtype=np.int32))
             for h, w, n in ((5, 7, 2), (4, 3, 0), (6, 6, 3))]
    packed, desc, boxes, labels, counts = collate_frames(items)
    assert list(counts) == [2, 0, 3] and boxes.shape == (5, 4) and labels.shape == (5,)
    for (f, _, _), (o, h, w) in zip(items, desc.numpy()):
        assert np.array_equal(packed.numpy()[o:o + h * w * 3].reshape(h, w, 3), f)


def test_the_test_pipeline_is_the_resize_alone():
    p = _pipe(TEST)
    assert not p.random and p.size == (300, 300)
    assert _pipe().random


@pytest.mark.parametrize('steps, word', [
    ([dict(type='Pad', size_divisor=32)], 'Pad'),
    ([dict(type='RandomCrop', crop_size=(10, 10))], 'RandomCrop'),
    ([dict(type='Resize', img_scale=(300, 300), keep_ratio=True)], 'keep_ratio'),
    ([dict(type='Resize', img_scale=(512, 300), keep_ratio=False)], 'img_scale'),
    ([dict(type='Resize', img_scale=[(300, 300), (200, 200)], keep_ratio=False)], 'img_scale'),
    ([dict(type='Resize', img_scale=(300, 300), keep_ratio=False, multiscale_mode='range')], 'multiscale_mode'),
    ([dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[1, 1, 1], to_rgb=True)], 'Normalize'),
    ([dict(type='Expand', mean=(123, 116, 103), ratio_range=(1, 3))], 'mean'),
    ([dict(type='RandomFlip', flip_ratio=0.5, direction='vertical')], 'direction'),
    ([dict(type='Albu', transforms=[dict(type='ShiftScaleRotate', p=0.5)])], 'ShiftScaleRotate'),
    ([dict(type='MultiScaleFlipAug', img_scale=(300, 300), flip=True, transforms=[])], 'flip'),
    ([dict(type='PhotoMetricDistortion', gamma=2)], 'gamma'),
    ([dict(type='RandomFlip', flip_ratio=0.5), dict(type='Resize', img_scale=(300, 300), keep_ratio=False)], 'order'),
    ([dict(type='LoadAnnotations', with_bbox=True, with_mask=True)], 'with_mask'),
    ([dict(type='Albu', transforms=[], bbox_params=dict(type='BboxParams', format='pascal_voc', min_visibility=0.3))], 'min_visibility'),
    ([dict(type='Albu', transforms=[], bbox_params=dict(type='BboxParams', format='coco'))], 'format'),
    ([dict(type='Albu', transforms=[], keymap=dict(img='image'))], 'keymap'),
    ([dict(type='Albu', transforms=[], update_pad_shape=True)], 'update_pad_shape'),
    ([dict(type='Collect', keys=['img', 'gt_masks'])], 'gt_masks'),
    ([dict(type='ImageToTensor', keys=['img', 'proposals'])], 'proposals'),
    ([dict(type='RandomFlip', flip_ratio=[0.3, 0.3], direction='horizontal')], 'flip_ratio'),
    ([dict(type='Expand', ratio_range=(1, 3), prob='often')], 'prob'),
])
def test_unknown_types_and_settings_are_refused_by_name(steps, word):
    with pytest.raises(NotImplementedError, match=word):
        _pipe(steps)
