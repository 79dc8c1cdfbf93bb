"""GPU: `t3d_jpeg_decode_u8` (csrc/jpeg.hip) bit for bit against the numpy restatement tests/jpeg_ref.py -- and against Pillow
where Pillow is libjpeg-turbo -- in ONE batched call over the whole matrix of sizes, samplings and qualities (mixed sizes, the
dw <= 2 images, 1 x 1, ragged MCUs on both edges), for several segment lengths, with guard bytes around every output slot and
around the workspace; the argument checks; and `GpuDetectionLoader` with `decode='device'` against the host-decoded loader."""
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

import jpeg_cases as C
import jpeg_ref as R

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
_ref = None


def reference():
    """[h, w, 3] per file of the matrix, by the restatement; computed once."""
    global _ref
    if _ref is None:
        _ref = [R.decode(d) for _, d in C.matrix()]
    return _ref


def run(datas, seg_mcus, guard=GUARD):
    """One t3d_jpeg_decode_u8 call over `datas` with `guard` bytes of FILL in front of and behind every output slot and the
    workspace.  -> (frames [h, w, 3] per file, status, guards untouched)."""
    from torchdet3d import _native as N
    from torchdet3d.dataloaders import jpeg as J
    rows = []
    for d in datas:
        rc, info, segs = J.index_jpeg(d, seg_mcus)
        assert rc == 0
        rows.append((info, segs))
    sizes = np.array([len(d) for d in datas], np.int64)
    frame = np.array([int(i['h']) * int(i['w']) * 3 for i, _ in rows], np.int64)
    out_off = guard + np.cumsum(frame + guard) - (frame + guard)               # odd offsets too: both store paths run
    plan = J.plan_batch(rows, np.cumsum(sizes) - sizes, sizes, out_off)
    dev = [torch.from_numpy(np.frombuffer(b''.join(datas), np.uint8).copy()).cuda()]
    dev += [torch.from_numpy(plan[k].view(np.uint8).copy()).cuda() for k in ('infos', 'segs', 'items')]
    out = torch.full((int(out_off[-1] + frame[-1] + guard),), FILL, dtype=torch.uint8, device='cuda')
    nbytes = ctypes.c_longlong(0)
    assert N.lib().t3d_jpeg_decode_work_bytes(plan['total_blocks'], ctypes.byref(nbytes)) == 0
    assert nbytes.value == plan['total_blocks'] * 192
    arena = torch.full((nbytes.value + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    work = arena[GUARD:GUARD + nbytes.value]                                   # (16-byte aligned, as the call demands)
    status = torch.full((len(datas),), 77, dtype=torch.int32, device='cuda')
    N.call('t3d_jpeg_decode_u8', N.ptr(dev[0]), dev[0].numel(), N.ptr(dev[1]), N.ptr(dev[2]), plan['total_segs'], N.ptr(dev[3]),
           N.ptr(out), out.numel(), work.data_ptr(), nbytes.value, plan['total_blocks'], N.ptr(status), len(datas), plan['max_segs'],
           plan['max_blocks'], N.stream())
    torch.cuda.synchronize()
    o, a = out.cpu().numpy(), arena.cpu().numpy()
    mask = np.ones(len(o), bool)
    frames = []
    for (info, _), off, n in zip(rows, out_off, frame):
        frames.append(o[off:off + n].reshape(int(info['h']), int(info['w']), 3))
        mask[off:off + n] = False
    clean = bool(np.all(o[mask] == FILL) and np.all(a[:GUARD] == FILL) and np.all(a[GUARD + nbytes.value:] == FILL))
    return frames, status.cpu().numpy(), clean


def test_one_batched_call_over_the_matrix_equals_the_restatement_and_pillow():
    from torchdet3d.dataloaders.jpeg import DEFAULT_SEG_MCUS
    datas = [d for _, d in C.matrix()]
    frames, status, clean = run(datas, DEFAULT_SEG_MCUS)
    assert not status.any(), status
    assert clean, 'a byte outside the output slots or the workspace was written'
    for (name, d), got, want in zip(C.matrix(), frames, reference()):
        assert np.array_equal(got, want), name
    if features.check_feature('libjpeg_turbo'):
        for (name, d), got in zip(C.matrix(), frames):
            assert np.array_equal(got, C.pillow(d)), name


@pytest.mark.parametrize('seg_mcus', [1, 3, 1 << 20])
def test_every_segment_length_gives_the_same_pixels(seg_mcus):
    datas = [d for _, d in C.matrix()]
    frames, status, clean = run(datas, seg_mcus, guard=61)                     # (an odd guard: other alignments of the slots)
    assert not status.any() and clean
    for (name, _), got, want in zip(C.matrix(), frames, reference()):
        assert np.array_equal(got, want), name


def test_several_workgroups_a_wave_and_aligned_frames():
    """A frame large enough for more than one entropy workgroup per image (more than 64 segments), more than one IDCT and
    colour workgroup, and dword-aligned output slots (guard 64, sizes that are multiples of 4)."""
    datas = [C.encode(C.image(136, 200, 3), '420', 90), C.encode(C.image(72, 96, 4), '444', 75), C.encode(C.image(64, 64, 5), 'gray', 50)]
    frames, status, clean = run(datas, 1)
    assert not status.any() and clean
    for d, got in zip(datas, frames):
        assert np.array_equal(got, R.decode(d))


def test_decode_jpeg_batch_is_the_collate_layout():
    from torchdet3d.dataloaders import collate_frames, decode_jpeg_batch, index_jpeg
    picked = [d for n, d in C.matrix() if '_q90_' in n][::7]
    rows = [index_jpeg(d)[1:] for d in picked]
    packed, desc = decode_jpeg_batch(picked, rows)
    torch.cuda.synchronize()
    want = collate_frames([(R.decode(d), np.zeros((0, 4), np.float32), np.zeros(0, np.int32)) for d in picked])
    assert np.array_equal(desc, want[1].numpy()) and np.array_equal(packed.cpu().numpy(), want[0].numpy())
    assert not decode_jpeg_batch.last_status.cpu().numpy().any()


def test_an_empty_batch_and_bad_arguments_launch_nothing():
    from torchdet3d import _native as N
    from torchdet3d.dataloaders import jpeg as J
    d = C.matrix()[100][1]
    rc, info, segs = J.index_jpeg(d)
    plan = J.plan_batch([(info, segs)], [0], [len(d)], [0])
    t = [torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda()] + \
        [torch.from_numpy(plan[k].view(np.uint8).copy()).cuda() for k in ('infos', 'segs', 'items')]
    out = torch.zeros(int(info['h']) * int(info['w']) * 3, dtype=torch.uint8, device='cuda')
    work = torch.zeros(plan['total_blocks'] * 192 + 16, dtype=torch.uint8, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    good = [N.ptr(t[0]), t[0].numel(), N.ptr(t[1]), N.ptr(t[2]), plan['total_segs'], N.ptr(t[3]), N.ptr(out), out.numel(), N.ptr(work),
            plan['total_blocks'] * 192, plan['total_blocks'], N.ptr(status), 1, plan['max_segs'], plan['max_blocks']]
    fn = N.lib().t3d_jpeg_decode_u8
    before = N.launch_count()
    bad = {0: None, 2: None, 3: None, 5: None, 6: None, 8: None, 11: None, 1: 0, 4: 0, 7: 0, 10: 0, 12: -1, 13: 0, 14: 0,
           9: plan['total_blocks'] * 192 - 1}
    for k, v in bad.items():
        args = list(good)
        args[k] = v
        assert fn(*args, N.stream()) == -1, k
    args = list(good)
    args[8] = work.data_ptr() + 4                                            # a misaligned workspace
    assert fn(*args, N.stream()) == -1
    args = list(good)
    args[12] = 0
    assert fn(*args, N.stream()) == 0                                        # B == 0
    assert N.lib().t3d_jpeg_decode_work_bytes(-1, ctypes.byref(ctypes.c_longlong(0))) == -1
    assert N.lib().t3d_jpeg_decode_work_bytes(1, None) == -1
    assert N.launch_count() == before
    assert fn(*good, N.stream()) == 0 and N.launch_count() == before + 3
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(int(info['h']), int(info['w']), 3), R.decode(d)) and status.item() == 0


# ---- the loader: decode='device' against the host-decoded loader ------------------------------------------------------------
from test_gpu_detect_augment import TEST, TRAIN, _with_size      # noqa: E402  (the config's pipelines at a small size)


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


def _cfg(root, decode=None, index=None):
    data = dict(samples_per_gpu=4, workers_per_gpu=0,
                train=dict(type='RepeatDataset', times=1,
                           dataset=dict(type='CocoDataset', classes=None, min_size=17, img_prefix=root,
                                        ann_file=os.path.join(root, 'annotations/objectron_train.json'))),
                val=dict(type='CocoDataset', img_prefix=root, test_mode=True, ann_file=os.path.join(root, 'annotations/objectron_test.json')))
    if decode is not None:
        data.update(decode=decode, decode_index=index, decode_seg_mcus=2)
    return dict(input_size=24, train_pipeline=_with_size(TRAIN, 24), test_pipeline=_with_size(TEST, 24), seed=7, data=data)


def _ref_decode(path):
    """The host loader's decoder in these tests: the restatement, so that the comparison does not depend on Pillow's flavour
    (a file the restatement does not take -- the progressive one -- is Pillow's on both sides)."""
    with open(path, 'rb') as f:
        data = f.read()
    try:
        return R.decode(data)
    except ValueError:
        return C.pillow(data)


def _loaders(root, tmp):
    from torchdet3d.builders import build_detection_loader
    host = build_detection_loader(_cfg(root))
    for l in host:
        l.dataset._decode_host = _ref_decode
    return host, build_detection_loader(_cfg(root, 'device', os.path.join(tmp, 'idx')))


def _epoch(loader, epoch):
    if hasattr(loader.sampler, 'set_epoch'):
        loader.sampler.set_epoch(epoch)
    out = [tuple(t.cpu().numpy() for t in b) for b in loader]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert u.dtype == v.dtype and np.array_equal(u, v)


@pytest.mark.parametrize('with_progressive', [False, True])
def test_the_device_decoded_loader_yields_the_host_decoded_batches(tmp_path, with_progressive):
    files = [C.encode(C.image(*((40, 56) if i % 2 == 0 else (33, 17)), 50 + i), ('420', '444', 'gray')[i % 3], 90) for i in range(10)]
    if with_progressive:
        files[5] = C.encode(C.image(33, 17, 99), '420', 90, progressive=True)
    root = str(tmp_path / 'frames')
    _write(root, files)
    (train_h, val_h), (train_d, val_d) = _loaders(root, str(tmp_path))
    assert train_d.decode == 'device' and train_h.decode == 'host' and len(train_d) == 2
    assert os.path.exists(str(tmp_path / 'idx.train.npy')) and os.path.exists(str(tmp_path / 'idx.val.npy'))
    assert list(train_d.dataset.index.reason) == [0] * 5 + [1 if with_progressive else 0] + [0] * 4
    for prefetch in (1, 0):
        train_h.prefetch = train_d.prefetch = val_h.prefetch = val_d.prefetch = prefetch
        e0 = _epoch(train_d, 0)
        _same(e0, _epoch(train_h, 0))
        e1 = _epoch(train_d, 1)
        _same(e1, _epoch(train_h, 1))
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(e0, e1)), 'two epochs gave the same images'
        v = _epoch(val_d, 0)
        _same(v, _epoch(val_h, 0))
        assert [len(b[0]) for b in v] == [4, 4, 2] and len(v[0]) == 5
        assert not train_d.last_status.cpu().numpy().any() and not val_d.last_status.cpu().numpy().any()
    # a second build loads the saved indexes instead of building them
    (_, _), (again, _) = _loaders(root, str(tmp_path))
    assert isinstance(again.dataset.index.infos, np.memmap)
    _same(_epoch(again, 0), e0)
