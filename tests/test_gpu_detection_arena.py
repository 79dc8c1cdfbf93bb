"""GPU: `build_detection_loader` with `data.cache = 'device'` (torchdet3d/dataloaders/detection_arena.py) against the
host-decoding loader over the same folder -- the same batches bit for bit, train and val, with and without files that take
the arena's host-decoded path -- and two steps of `DetectorTrainer.train` from either loader: the same losses bit for bit.
The folder, the config and the reference decoder are those of tests/test_gpu_jpeg.py (copied, not imported)."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import detect_draw_cases as K
import jpeg_cases as C
import jpeg_ref as R

pytestmark = pytest.mark.gpu

TEST = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(24, 24), flip=False,
         transforms=[dict(type='Resize', keep_ratio=False), dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
                     dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]),
]


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


def _cfg(root, size=24, bs=4, cache=None, index=None):
    data = dict(samples_per_gpu=bs, workers_per_gpu=0,
                train=dict(type='RepeatDataset', times=1,
                           dataset=dict(type='CocoDataset', classes=None, min_size=17, img_prefix=root,
                                        ann_file=os.path.join(root, 'annotations/objectron_train.json'))),
                val=dict(type='CocoDataset', img_prefix=root, test_mode=True, ann_file=os.path.join(root, 'annotations/objectron_test.json')))
    if cache is not None:
        data.update(cache=cache, decode_index=index, decode_seg_mcus=2)
    return dict(input_size=size, train_pipeline=_with_size(K.CONFIG, size), test_pipeline=_with_size(TEST, size), seed=7, data=data)


def _ref_decode(path):
    """The host loader's decoder in these tests: the restatement, so that the comparison does not depend on Pillow's flavour
    (a file the restatement does not take -- progressive, 4:2:2 -- is Pillow's on both sides)."""
    with open(path, 'rb') as f:
        data = f.read()
    try:
        return R.decode(data)
    except ValueError:
        return C.pillow(data)


def _loaders(root, tmp, **kw):
    from torchdet3d.builders import build_detection_loader
    host = build_detection_loader(_cfg(root, **kw))
    for l in host:
        l.dataset._decode_host = _ref_decode
    return host, build_detection_loader(_cfg(root, cache='device', index=os.path.join(tmp, 'idx'), **kw))


def _epoch(loader, epoch):
    if hasattr(loader.sampler, 'set_epoch'):
        loader.sampler.set_epoch(epoch)
    out = [tuple(t.cpu().numpy() for t in b) for b in loader]
    torch.cuda.synchronize()
    return out


def _same(arena, host):
    """The arena loader's tuples against the host loader's: images, counts, labels (and ori_shapes) bit for bit, boxes bit for
    bit on the host's leading G columns, zero behind them."""
    assert len(arena) == len(host) > 0
    for a, h in zip(arena, host):
        assert len(a) == len(h)
        G = h[1].shape[1]
        assert a[1].shape[1] >= G and a[1].shape[1] == a[2].shape[1]
        assert a[0].dtype == h[0].dtype and np.array_equal(a[0], h[0])
        assert a[1].dtype == h[1].dtype and a[1][:, :G].tobytes() == h[1].tobytes() and not a[1][:, G:].view(np.uint32).any()
        assert a[2].dtype == h[2].dtype and np.array_equal(a[2][:, :G], h[2]) and not a[2][:, G:].any()
        for u, v in zip(a[3:], h[3:]):
            assert u.dtype == v.dtype and np.array_equal(u, v)


def _files(with_host_decoded):
    files = [C.encode(C.image(*((40, 56) if i % 2 == 0 else (33, 17)), 50 + i), ('420', '444', 'gray')[i % 3], 90) for i in range(10)]
    if with_host_decoded:
        files[5] = C.encode(C.image(33, 17, 99), '420', 90, progressive=True)
        files[8] = C.encode(C.image(40, 56, 98), '422', 90)
    return files


@pytest.mark.parametrize('with_host_decoded', [False, True])
def test_the_arena_loader_yields_the_host_decoded_batches(tmp_path, with_host_decoded):
    from torchdet3d.dataloaders import ArenaDetectionLoader
    root = str(tmp_path / 'frames')
    _write(root, _files(with_host_decoded))
    (train_h, val_h), (train_a, val_a) = _loaders(root, str(tmp_path))
    assert isinstance(train_a, ArenaDetectionLoader) and isinstance(val_a, ArenaDetectionLoader) and len(train_a) == len(train_h) == 2
    assert len(val_a) == len(val_h) == 3 and train_a.batch_size == 4 and train_a.dataset is train_a.arena.frames
    assert os.path.exists(str(tmp_path / 'idx.train.npy')) and os.path.exists(str(tmp_path / 'idx.val.npy'))
    want_kind = [0] * 10
    if with_host_decoded:
        want_kind[5] = want_kind[8] = 1
    G = max(len(l) for l in train_a.arena.frames._labels)
    assert list(train_a.arena.kind) == want_kind and train_a.arena.G == G == val_a.arena.G
    for prefetch in (1, 0):
        train_h.prefetch = train_a.prefetch = val_h.prefetch = val_a.prefetch = prefetch
        e0 = _epoch(train_a, 0)
        _same(e0, _epoch(train_h, 0))
        assert not train_a.last_status.cpu().numpy().any()
        e1 = _epoch(train_a, 1)
        _same(e1, _epoch(train_h, 1))
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(e0, e1)), 'two epochs gave the same images'
        v = _epoch(val_a, 0)
        _same(v, _epoch(val_h, 0))
        assert [len(b[0]) for b in v] == [4, 4, 2] and len(v[0]) == 5 and v[0][1].shape[1] == G
        assert not train_a.last_status.cpu().numpy().any() and not val_a.last_status.cpu().numpy().any()


def test_a_fill_of_more_chunks_than_staging_buffers_keeps_every_files_bytes(tmp_path, monkeypatch):
    """`DetectionArena.fill` with one file a chunk: ten chunks through three pinned buffers, behind a stream that is running
    late, so a buffer rewritten before its upload has run would put a later file's bytes in an earlier file's place."""
    from torchdet3d.dataloaders import DetectionArena, ObjectronFrames
    root = str(tmp_path / 'frames')
    _write(root, _files(True))
    fr = ObjectronFrames(root, 'val', decode='device')
    fr.build_index(seg_mcus=2)
    arena = DetectionArena(fr)
    assert len(arena) == 10 >= 3 + 2 and list(np.flatnonzero(arena.kind)) == [5, 8]       # (three buffers rotate)
    want = []
    for i, name in enumerate(fr.files):
        path = os.path.join(root, name)
        want.append(fr._decode_host(path).reshape(-1) if arena.kind[i] else np.fromfile(path, np.uint8))
    assert [len(w) for w in want] == list(arena.size)
    monkeypatch.setattr(DetectionArena, 'STAGING', int(arena.size.min()))                 # below any two files: every chunk is one file
    torch.cuda._sleep(100_000_000)
    arena.fill()
    torch.cuda.synchronize()
    total = int(arena.size.sum())
    assert arena.data.numel() >= total and np.array_equal(arena.data[:total].cpu().numpy(), np.concatenate(want))


def test_two_train_steps_from_the_arena_give_the_host_loaders_losses(tmp_path):
    """The smallest detector configuration of tests/test_gpu_detector_train.py: SSD300 at 300 x 300, batches of 2, bf16 storage."""
    from torchdet3d.models.ssd import SSD300
    from torchdet3d.trainer import DetectorTrainer
    root = str(tmp_path / 'frames')
    _write(root, _files(False)[:4])
    (train_h, _), (train_a, _) = _loaders(root, str(tmp_path), size=300, bs=2)
    losses = []
    for loader in (train_h, train_a):
        tr = DetectorTrainer(SSD300(device='cuda:0', dtype=torch.bfloat16, seed=0), warmup_iters=4)
        step, got = tr.train_step, []
        tr.train_step = lambda *a, **k: got.append(step(*a, **k)) or got[-1]
        tr.train(loader, 0)
        torch.cuda.synchronize()
        losses.append([[float(x) for x in t] for t in got])
    assert len(losses[0]) == 2 and all(np.isfinite(x) for t in losses[0] for x in t)
    assert losses[0] == losses[1], losses
