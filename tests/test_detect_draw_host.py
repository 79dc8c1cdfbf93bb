"""CPU: `t3d_detect_draw_host` (csrc/detect_draw.h run on the CPU) against the numpy pipeline it restates --
`DetectionAugmentPipeline.draw` / `.boxes` / `.records` -- bit for bit over the cases of tests/detect_draw_cases.py; the arena's
batch planning against `plan_batch`; the `data.cache` key of `build_detection_loader` without a GPU."""
import io
import json
import os

import numpy as np
import pytest

import detect_draw_cases as K

PER_CASE = {K.TINY: 400}            # samples of a case (200 otherwise): 13 cases, 2 800 samples


def _check(case, B, got, want):
    rec, gb, gl, gc, diag = got
    wrec, wb, wl, wmode, wdrawn = want
    name = case['name']
    assert rec.tobytes() == wrec.tobytes(), name
    assert np.array_equal(gc, [len(l) for l in wl]), name
    modes = K.pipeline(case).crop['modes'] if K.pipeline(case).crop is not None else None
    for i in range(B):
        n = len(wl[i])
        assert gb[i, :n].tobytes() == np.asarray(wb[i], np.float32).tobytes(), (name, i)
        assert np.array_equal(gl[i, :n], wl[i]), (name, i)
        assert not gb[i, n:].view(np.uint32).any() and not gl[i, n:].any(), (name, i)
        assert (1.0 if modes is None else modes[diag[i, 0]]) == wmode[i] and (modes is not None or diag[i, 0] == -1), (name, i)
    assert np.array_equal(diag[:, 1], wdrawn), name


@pytest.fixture(scope='module')
def results():
    """Per case: (B, the host entry's outputs, the numpy pipeline's) -- computed once."""
    from torchdet3d.dataloaders.detection_arena import detect_draw_host
    out = {}
    for case in K.cases():
        B = PER_CASE.get(case['name'], 200)
        frames, boxes, labels, start = K.tables(case, B)
        out[case['name']] = (case, B, detect_draw_host(K.pipeline(case), case['key'], frames, boxes, labels, start, case['G']),
                             K.host_reference(case, B))
    return out


def test_the_host_entry_equals_the_numpy_pipeline_bit_for_bit(results):
    assert sum(B for _, B, _, _ in results.values()) >= 2000
    for case, B, got, want in results.values():
        _check(case, B, got, want)


def test_the_tiny_box_case_restarts_the_mode_loop_and_reaches_mode_one(results):
    """A mode's 50 tries draw at most 1 + 50 * 4 = 201 uniforms: more than that is a restart of the outer loop."""
    case, B, got, want = results[K.TINY]
    drawn, mode_at = got[4][:, 1], got[4][:, 0]
    assert np.mean(drawn > 201) >= 0.25, np.mean(drawn > 201)
    assert np.any(mode_at == 0) and K.pipeline(case).crop['modes'][0] == 1.0
    assert np.mean(want[4] > 201) >= 0.25                                   # (the host's own search: the same statement)


def test_the_cases_reach_every_branch(results):
    rec = np.concatenate([r[2][0] for r in results.values()])
    assert set(rec['turns']) == {0, 1, 3} and set(rec['flags'] & 1) == {0, 1} and (rec['left'] > 0).any() and (rec['top'] > 0).any()
    assert len({tuple(p) for p in rec['perm']}) == 6
    modes = np.concatenate([r[2][4][:, 0] for r in results.values()])
    assert set(modes) == set(range(-1, 7))
    case, B, got, _ = results['config/100x130/cap']
    assert got[3].max() == 64 == case['G'] and got[3].min() < 64              # capacity, and a search that dropped boxes
    assert any(len(K.cases()[i]['key']) == 4 and K.cases()[i]['key'][0] >= 2 ** 32 for i in range(len(K.cases())))


def test_bad_samples_and_arguments():
    import ctypes

    from torchdet3d import _native as N
    from torchdet3d.dataloaders.detection_arena import detect_draw_host, key_words, pipeline_cfg
    case = K.cases()[1]
    frames, boxes, labels, start = K.tables(case, 4)
    good = detect_draw_host(K.pipeline(case), case['key'], frames, boxes, labels, start, 2)
    bad = frames.copy()
    bad[1, 3] = 1                                               # an index behind the table
    bad[2, 1] = 0                                               # no rows
    got = detect_draw_host(K.pipeline(case), case['key'], bad, boxes, labels, start, 2)
    for k in (1, 2):
        assert not got[0][k:k + 1].tobytes().strip(b'\0') and got[3][k] == 0 and not got[1][k].any() and not got[2][k].any()
        assert tuple(got[4][k]) == (-1, 0)
    for k in (0, 3):
        assert all(np.array_equal(g[k], w[k]) for g, w in zip(got, good))
    start_bad = np.array([0, 5], np.int64)                      # a box range behind the table
    got = detect_draw_host(K.pipeline(case), case['key'], frames, boxes, labels, start_bad, 2)
    assert not got[3].any() and not got[0].tobytes().strip(b'\0')
    # argument errors
    cfg, words = pipeline_cfg(K.pipeline(case)), key_words(case['key'])
    rec, gb, gl = np.zeros(4 * 80, np.uint8), np.zeros((4, 2, 4), np.float32), np.zeros((4, 2), np.int32)
    gc, diag = np.zeros(4, np.int32), np.zeros((4, 2), np.int32)
    args = [cfg.ctypes.data, len(cfg), words.ctypes.data, len(words), frames.ctypes.data, 4, boxes.ctypes.data, labels.ctypes.data,
            start.ctypes.data, 1, 1, 2, rec.ctypes.data, gb.ctypes.data, gl.ctypes.data, gc.ctypes.data, diag.ctypes.data, None]
    fn = N.lib().t3d_detect_draw_host
    assert fn(*args) == 0
    for k, v in {0: None, 2: None, 4: None, 6: None, 7: None, 8: None, 12: None, 13: None, 14: None, 15: None, 16: None, 1: 33, 3: 17,
                 5: -1, 11: 0}.items():
        a = list(args)
        a[k] = v
        assert fn(*a) == N.ERR_ARG, k
    no_whole = cfg.copy()
    no_whole[15] = 0.2                                          # a crop without the mode that always returns
    args[0] = no_whole.ctypes.data
    assert fn(*args) == N.ERR_ARG
    assert list(key_words((2 ** 32 + 5, 0, 1, 70000))) == [5, 1, 0, 1, 70000]
    assert ctypes.sizeof(ctypes.c_double) * len(cfg) == 34 * 8


# ---- arena planning, pure numpy ---------------------------------------------------------------------------------------------
def _jpeg(h, w, seed, sampling='420', **kw):
    import jpeg_cases as C
    return C.encode(C.image(h, w, seed), sampling, 90, **kw)


def test_the_arena_plan_equals_plan_batch_apart_from_the_resident_offsets():
    from torchdet3d.dataloaders import jpeg as J
    from torchdet3d.dataloaders.detection_arena import plan_arena_batch
    files = [_jpeg(*((40, 56) if i % 2 == 0 else (33, 17)), 50 + i, ('420', '444', 'gray')[i % 3]) for i in range(7)]
    rows = [J.index_jpeg(f, 2)[1:] for f in files]
    infos = np.array([r[0] for r in rows], J.INFO_DTYPE)
    size = np.array([len(f) for f in files], np.int64)
    nseg = infos['nseg'].astype(np.int64)
    seg_start = np.cumsum(nseg) - nseg
    blocks = infos['mcus_x'].astype(np.int64) * infos['mcus_y'] * np.array(J._BLOCKS_PER_MCU)[infos['sampling']]
    idx = np.array([5, 0, 6, 2, 2])
    got = plan_arena_batch(idx, np.cumsum(size) - size, size, seg_start, infos['h'], infos['w'], blocks, nseg)
    fb = np.array([int(infos['h'][i]) * int(infos['w'][i]) * 3 for i in idx], np.int64)
    bs = size[idx]
    want = J.plan_batch([rows[i] for i in idx], np.cumsum(bs) - bs, bs, np.cumsum(fb) - fb)
    for f in ('file_bytes', 'out_offset', 'block_offset', 'reserved'):
        assert np.array_equal(got['items'][f], want['items'][f]), f
    assert np.array_equal(got['items']['file_offset'], (np.cumsum(size) - size)[idx])
    assert np.array_equal(got['items']['seg_offset'], seg_start[idx])
    for f in ('total_blocks', 'max_segs', 'max_blocks'):
        assert got[f] == want[f], f
    assert got['out_bytes'] == fb.sum() and np.array_equal(got['frames'], np.stack([np.cumsum(fb) - fb, infos['h'][idx], infos['w'][idx], idx], 1))
    # the resident segment rows an item points at are the rows plan_batch concatenates
    segs = np.concatenate([r[1] for r in rows])
    for k, i in enumerate(idx):
        a, b = int(got['items']['seg_offset'][k]), int(want['items']['seg_offset'][k])
        assert segs[a:a + nseg[i]].tobytes() == want['segs'][b:b + nseg[i]].tobytes()


# ---- the builder's keys, without a GPU --------------------------------------------------------------------------------------
def _write(root, files):
    from PIL import Image
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    images, anns = [], []
    for i, data in enumerate(files):
        fn = f'images/{i:03d}.jpg'
        with open(os.path.join(root, fn), 'wb') as f:
            f.write(data)
        w, h = Image.open(io.BytesIO(data)).size
        images.append(dict(id=i + 1, file_name=fn, width=w, height=h))
        anns.append(dict(id=i, image_id=i + 1, category_id=1 + i % 9, iscrowd=0, bbox=[2.0, 3.0, w * .4, h * .5]))
    for name in ('objectron_train.json', 'objectron_test.json'):
        with open(os.path.join(root, 'annotations', name), 'w') as f:
            json.dump(dict(images=images, annotations=anns, categories=[]), f)


def _cfg(root, **data):
    d = dict(samples_per_gpu=2, workers_per_gpu=0,
             train=dict(type='RepeatDataset', times=1,
                        dataset=dict(type='CocoDataset', classes=None, min_size=17, img_prefix=root,
                                     ann_file=os.path.join(root, 'annotations/objectron_train.json'))),
             val=dict(type='CocoDataset', img_prefix=root, test_mode=True, ann_file=os.path.join(root, 'annotations/objectron_test.json')))
    d.update(data)
    test = [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', img_scale=(300, 300), flip=False,
                                                 transforms=[dict(type='Resize', keep_ratio=False), dict(type='Collect', keys=['img'])])]
    return dict(input_size=300, train_pipeline=K.CONFIG, test_pipeline=test, seed=7, data=d)


def test_the_cache_key_of_the_builder_without_a_gpu(tmp_path):
    import torch

    from torchdet3d.builders import build_detection_loader
    from torchdet3d.dataloaders import ObjectronFrames
    from torchdet3d.dataloaders.detection_arena import DetectionArena
    root = str(tmp_path / 'frames')
    _write(root, [_jpeg(40, 56, 1), _jpeg(33, 17, 2, '444'), _jpeg(40, 56, 3, 'gray'), _jpeg(33, 17, 4, progressive=True)])
    with pytest.raises(ValueError, match='data.cache'):
        build_detection_loader(_cfg(root, cache='host'))
    with pytest.raises(ValueError, match=r'need \d+ bytes .* over the budget data.cache_max_gb = 1e-06 \(1073 bytes\)'):
        build_detection_loader(_cfg(root, cache='device', cache_max_gb=1e-6))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            build_detection_loader(_cfg(root, cache='device'))
    # the plan is host only: sizes, the host-decoded file as its frame, the capacity
    ds = ObjectronFrames(root, 'train', decode='device')
    ds.build_index(seg_mcus=2)
    arena = DetectionArena(ds)
    assert arena.data is None and arena.G == 1 and list(arena.kind) == [0, 0, 0, 1]
    assert arena.size[3] == 33 * 17 * 3 and (arena.h[3], arena.w[3]) == (33, 17)
    assert np.array_equal(arena.size[:3], ds.index.size[:3]) and np.array_equal(arena.file_off, np.cumsum(arena.size) - arena.size)
    ds._boxes[0] = np.zeros((65, 4), np.float32)
    ds._labels[0] = np.zeros(65, np.int32)
    with pytest.raises(ValueError, match='65 boxes'):
        DetectionArena(ds)
    # a stale file raises, by the index's own check
    os.utime(os.path.join(root, ds.files[1]), ns=(1, 1))
    ds._boxes[0], ds._labels[0] = ds._boxes[0][:1], ds._labels[0][:1]
    with pytest.raises(RuntimeError, match='changed since it was indexed'):
        DetectionArena(ds)
