"""GPU: `t3d_detect_roi_plan` (csrc/detect_roi.hip) equals `t3d_detect_roi_plan_host` -- the same header on the CPU, which
tests/test_detect_roi_plan_host.py holds to numpy -- byte for byte over the inputs of tests/detect_roi_cases.py, every output
between guard bytes; and `ArenaDetectionLoader(crop_decode=True)` (`data.decode_crop`), which decodes of every frame only what
its drawn crop reads, against the same loader with the flag off over the same folders: the same batches bit for bit.
The folder and the config are those of tests/test_gpu_detection_arena.py (copied, not imported)."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import detect_draw_cases as K
import detect_roi_cases as R
import jpeg_cases as C

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5

TEST = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(24, 24), flip=False,
         transforms=[dict(type='Resize', keep_ratio=False), dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
                     dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]),
]


# ---- the planner: device against host twin --------------------------------------------------------------------------------------
def _device(rec, infos, items, src_bytes, sample=None):
    """One t3d_detect_roi_plan call -> ((records, roi items, rects, diag) as numpy, guards untouched)."""
    from torchdet3d import _native as N
    from torchdet3d.dataloaders import jpeg as J
    n, B = len(items), len(rec)
    d_infos, d_items = (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (infos, items))
    d_sample = None if sample is None else torch.from_numpy(np.ascontiguousarray(sample, np.int32)).cuda()
    sizes = [B * 80, n * 48, n * 48, n * 8]
    outs = [torch.full((s + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda') for s in sizes]
    outs[0][GUARD:GUARD + sizes[0]] = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()       # records: in and out
    N.call('t3d_detect_roi_plan', outs[0].data_ptr() + GUARD, B, None if sample is None else N.ptr(d_sample), N.ptr(d_infos), N.ptr(d_items),
           n, int(src_bytes), *[o.data_ptr() + GUARD for o in outs[1:]], N.stream())
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    clean = all(np.all(h[:GUARD] == FILL) and np.all(h[GUARD + s:] == FILL) for h, s in zip(host, sizes))
    body = [h[GUARD:GUARD + s].copy() for h, s in zip(host, sizes)]
    return (body[0].view(rec.dtype), body[1].view(J.ITEM_DTYPE), body[2].view(np.int32).reshape(n, 12), body[3].view(np.int32).reshape(n, 2)), clean


@pytest.mark.parametrize('sampling', R.SAMPLINGS)
def test_the_device_planner_equals_the_host_twin(sampling):
    from torchdet3d.dataloaders.detection_arena import detect_roi_plan_host
    for case, rec, src_bytes in R.drawn().values():
        for seg_mcus in R.SEG_MCUS:
            data, info, _ = R.index_rows(case['h'], case['w'], sampling, seg_mcus)
            infos, items = np.array([info] * len(rec)), R.whole_items(len(rec), info, len(data))
            got, clean = _device(rec, infos, items, src_bytes)
            assert clean, f'{case["name"]}: a byte outside the outputs was written'
            for g, w in zip(got, detect_roi_plan_host(rec, infos, items, src_bytes)):
                assert g.tobytes() == w.tobytes(), (case['name'], sampling, seg_mcus)


def test_refused_records_the_sample_table_more_than_one_workgroup_and_an_empty_call():
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.detection_arena import detect_roi_plan_host
    case, rec, src_bytes = R.drawn()['config/100x130/mid']
    data, info, _ = R.index_rows(100, 130, '420', 2)
    bad = np.tile(rec, 4)[:150].copy()                  # 150 items: three workgroups, the last one ragged
    bad['turns'][0], bad['cx1'][1], bad['flags'][3], bad['h'][4] = 2, bad['cx0'][1], 128, 99
    bad['perm'][2] = (0, 0, 2)
    bad[5] = np.zeros(1, rec.dtype)[0]
    sample = np.arange(150, dtype=np.int32)[::-1].copy()
    sample[7], sample[8] = -1, 150                      # no record
    infos, items = np.array([info] * 150), R.whole_items(150, info, len(data))
    infos['seg_mcus'][9] = 0                            # a row the indexer would not write
    got, clean = _device(bad, infos, items, src_bytes, sample)
    assert clean
    for g, w in zip(got, detect_roi_plan_host(bad, infos, items, src_bytes, sample)):
        assert g.tobytes() == w.tobytes()
    same = [0, 1, 2, 3, 4, 5, 149 - 7, 149 - 8, 149 - 9]                   # refused, without an item, on a bad row: not touched
    assert got[0][same].tobytes() == bad[same].tobytes() and got[0][6].tobytes() != bad[6].tobytes()
    # nothing to plan launches nothing; an argument error neither
    before = N.launch_count()
    fn = N.lib().t3d_detect_roi_plan
    assert fn(None, 0, None, None, None, 0, 0, None, None, None, N.stream()) == 0
    assert fn(None, 4, None, None, None, 0, 100, None, None, None, N.stream()) == 0
    assert fn(None, 4, None, None, None, 2, 100, None, None, None, N.stream()) == N.ERR_ARG
    assert N.launch_count() == before


# ---- the loader: flag on against flag off ---------------------------------------------------------------------------------------
def _with_size(steps, s):
    out = []
    for st in steps:
        st = dict(st)
        if 'img_scale' in st:
            st['img_scale'] = (s, s)
        out.append(st)
    return out


def _write(root, files):
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    rng = np.random.default_rng(3)
    images, anns = [], []
    for i, data in enumerate(files):
        fn = f'images/{i:03d}.jpg'
        with open(os.path.join(root, fn), 'wb') as f:
            f.write(data)
        w, h = Image.open(io.BytesIO(data)).size
        images.append(dict(id=i + 1, file_name=fn, width=w, height=h))
        for _ in range(int(rng.integers(1, 4))):
            x, y = float(rng.uniform(0, w * .5)), float(rng.uniform(0, h * .5))
            anns.append(dict(id=len(anns), image_id=i + 1, category_id=int(rng.integers(1, 10)), iscrowd=0,
                             bbox=[x, y, float(rng.uniform(4, w * .45)), float(rng.uniform(4, h * .45))]))
    for name in ('objectron_train.json', 'objectron_test.json'):
        with open(os.path.join(root, 'annotations', name), 'w') as f:
            json.dump(dict(images=images, annotations=anns, categories=[]), f)


def _cfg(root, index, seg_mcus, size=24, bs=4, **more):
    data = dict(samples_per_gpu=bs, workers_per_gpu=0, cache='device', decode_index=index, decode_seg_mcus=seg_mcus,
                train=dict(type='RepeatDataset', times=1,
                           dataset=dict(type='CocoDataset', classes=None, min_size=17, img_prefix=root,
                                        ann_file=os.path.join(root, 'annotations/objectron_train.json'))),
                val=dict(type='CocoDataset', img_prefix=root, test_mode=True, ann_file=os.path.join(root, 'annotations/objectron_test.json')))
    data.update(more)
    return dict(input_size=size, train_pipeline=_with_size(K.CONFIG, size), test_pipeline=_with_size(TEST, size), seed=7, data=data)


def _files(kind):
    if kind == 'large':     # rectangles that span several MCU rows and start at odd MCU and chroma positions
        return [C.encode(C.image(*((100, 130) if i % 2 == 0 else (120, 200)), 70 + i), ('420', '444', 'gray')[i % 3], 90) for i in range(6)]
    files = [C.encode(C.image(*((40, 56) if i % 2 == 0 else (33, 17)), 50 + i), ('420', '444', 'gray')[i % 3], 90) for i in range(10)]
    if kind == 'host_decoded':
        files[5] = C.encode(C.image(33, 17, 99), '420', 90, progressive=True)
        files[8] = C.encode(C.image(40, 56, 98), '422', 90)
    return files


def _epoch(loader, epoch):
    """-> (the epoch's batches as numpy, every batch's status vector, every batch's planner diag or None)."""
    if hasattr(loader.sampler, 'set_epoch'):
        loader.sampler.set_epoch(epoch)
    status, diag, finish = [], [], loader._finish

    def noted(*a, **k):                                 # (with prefetch `last_status` runs ahead of the batch that is yielded)
        out = finish(*a, **k)
        status.append(loader.last_status)
        diag.append(loader.last_crop_diag)
        return out
    loader._finish = noted
    try:
        out = [tuple(t.cpu().numpy() for t in b) for b in loader]
    finally:
        del loader._finish
    torch.cuda.synchronize()
    assert len(status) == len(out)
    return out, [s.cpu().numpy() for s in status], [None if d is None else d.cpu().numpy() for d in diag]


def _equal(on, off):
    assert len(on) == len(off) > 0
    for a, b in zip(on, off):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


@pytest.mark.parametrize('seg_mcus', [1, 2])
@pytest.mark.parametrize('kind', ['baseline', 'host_decoded', 'large'])
def test_the_crop_decoding_loader_yields_the_whole_frame_loaders_batches(tmp_path, kind, seg_mcus):
    from torchdet3d.builders import build_detection_loader
    from torchdet3d.dataloaders import ArenaDetectionLoader, DetectionAugmentPipeline
    root = str(tmp_path / 'frames')
    _write(root, _files(kind))
    train, val = build_detection_loader(_cfg(root, str(tmp_path / 'idx'), seg_mcus, decode_crop=True))
    assert isinstance(train, ArenaDetectionLoader) and train.crop_decode and not val.crop_decode
    assert int(train.arena.kind.sum()) == (2 if kind == 'host_decoded' else 0)
    assert set(train.arena.frames.index.infos['seg_mcus'][train.arena.kind == 0]) == {seg_mcus}
    asked = {}
    for name, steps in K.PIPELINES.items():
        tf = DetectionAugmentPipeline(_with_size(steps, 24), (24, 24))
        off, on = (ArenaDetectionLoader(train.arena, tf, 4, sampler=train.sampler, drop_last=True, seed=7, rank=0, crop_decode=flag)
                   for flag in (False, True))
        pixels = 0
        for prefetch in (1, 0):
            off.prefetch = on.prefetch = prefetch
            for epoch in (0, 1):
                (got, st_on, diag), (want, st_off, none) = _epoch(on, epoch), _epoch(off, epoch)
                assert len(got) == len(train) == (1 if kind == 'large' else 2)
                _equal(got, want)
                assert not any(s.any() for s in st_on + st_off), (name, prefetch, epoch)
                assert none == [None] * len(want) and all(d.shape == (len(s), 2) and (d > 0).all() for d, s in zip(diag, st_on))
                pixels += sum(int(d[:, 0].sum()) for d in diag)
        asked[name] = pixels
    # Resize and flip alone read every frame whole; Expand and the crop leave parts of them unread
    assert asked['config'] < asked['resize_flip'] and asked['no_expand'] < asked['resize_flip'], asked
    # the test pipeline reads whole frames and ignores the flag
    flagged = ArenaDetectionLoader(val.arena, val.pipeline, 4, indices=range(len(val.arena)), seed=7, rank=0, dataset=val.dataset,
                                   crop_decode=True)
    for prefetch in (1, 0):
        flagged.prefetch = val.prefetch = prefetch
        (got, st_on, diag), (want, st_off, _) = _epoch(flagged, 0), _epoch(val, 0)
        _equal(got, want)
        assert len(got[0]) == 5 and not any(s.any() for s in st_on + st_off) and diag == [None] * len(got)
