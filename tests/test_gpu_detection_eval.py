"""GPU: `t3d_ssd_cap_per_image` and `t3d_coco_match` (csrc/detection_eval.hip) behind `DetectionEvaluator`, bit for bit
against the plain-loop restatement of COCOeval (tests/coco_eval_ref.py): the per-image cap, every rule of the matching on the
smallest scene that can get it wrong, random scenes with their own coverage asserted, determinism, the validation loop end to
end on an untrained and a briefly trained detector, and the argument checks."""
import json
import os

import numpy as np
import pytest
import torch

import coco_eval_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ('score', 'dtm', 'dtig', 'ndt', 'ngt', 'valid')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _evaluator(nc, rows, max_per_img=1000):
    from torchdet3d.evaluation import DetectionEvaluator
    return DetectionEvaluator(None, rows, num_classes=nc, max_per_img=max_per_img)


def _scene(images, nc, K, G, shapes=None, size=300):
    """images: [(dets {class: [(x1, y1, x2, y2, score)]}, gts [(x1, y1, x2, y2, label)])], boxes in input pixels."""
    B = len(images)
    out, cnt = np.zeros((B, nc, K, 6), F), np.zeros((B, nc), np.int32)
    gb, gl, gc = np.zeros((B, G, 4), F), np.zeros((B, G), np.int32), np.zeros(B, np.int32)
    for b, (dets, gts) in enumerate(images):
        for c, rows in dets.items():
            cnt[b, c] = len(rows)
            for i, r in enumerate(rows[:K]):
                out[b, c, i, :5] = r
                out[b, c, i, 5] = c
        gc[b] = len(gts)
        for g, (x1, y1, x2, y2, lab) in enumerate(gts):
            gb[b, g], gl[b, g] = (x1, y1, x2, y2), lab
    shapes = np.full((B, 2), size, np.int32) if shapes is None else np.asarray(shapes, np.int32)
    return out, cnt, gb, gl, gc, shapes


def _same(got, want, what=''):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5])


def _check(arrays, nc, size=(300, 300), max_per_img=1000):
    """One batch through a fresh evaluator; the record must equal the restatement's.  -> (record, evaluator)."""
    out, cnt, gb, gl, gc, shapes = arrays
    ev = _evaluator(nc, len(cnt), max_per_img)
    capped = ev.evaluate_detections(*[_dev(a) for a in arrays], input_size=size)
    got = ev.record()
    want, want_capped = R.record_of(out, cnt, gb, gl, gc, shapes, size[1], size[0], max_per_img)
    assert np.array_equal(capped.cpu().numpy(), want_capped)
    _same(got, want)
    return got, ev


def _bits(word, a):
    return (int(word) >> (10 * a)) & 0x3ff


# ---- the cap

def _cap(out, cnt, cap):
    from torchdet3d import _native as N
    B, nc, K = out.shape[:3]
    o, c = _dev(out), _dev(cnt)
    res = torch.full((B, nc), -7, dtype=torch.int32, device='cuda')
    N.call('t3d_ssd_cap_per_image', N.ptr(o), N.ptr(c), B, nc, K, cap, N.ptr(res), N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), out) and np.array_equal(c.cpu().numpy(), cnt)       # only read
    return res.cpu().numpy()


def test_cap_equals_the_numpy_rule():
    nc, K, cap = 3, 4, 5
    out = np.zeros((5, nc, K, 6), F)
    # scores tied across classes and within a class, every class in non-increasing order; rows past a count hold a
    # large score that must never be looked at
    out[..., 4] = 9.0
    cnt = np.array([[1, 2, 1], [2, 2, 1], [3, 4, 2], [0, 0, 0], [4, 9, -3]], np.int32)      # below, at, above, none, clamped
    tied = np.array([[.5, .5, .25, .25], [.75, .5, .5, .25], [.5, .5, .5, .125]], F)
    for b in range(5):
        for c in range(nc):
            n = min(max(cnt[b, c], 0), K)
            out[b, c, :n, 4] = tied[c, :n]
    want = np.stack([R.cap_counts(out[b], cnt[b], cap) for b in range(5)])
    assert list(want.sum(1)) == [4, 5, 5, 0, 5]
    assert np.array_equal(_cap(out, cnt, cap), want)
    assert np.array_equal(_cap(out, cnt, 0), np.zeros_like(want))
    assert np.array_equal(_cap(out, cnt, 1000), np.clip(cnt, 0, K))


def test_cap_on_random_rows_at_the_detectors_shape():
    rng = np.random.default_rng(5)
    B, nc, K = 3, 9, 200
    out = rng.random((B, nc, K, 6)).astype(F)
    out[..., 4] = -np.sort(-np.round(rng.random((B, nc, K)) * 64) / 64, axis=2)      # a 1/64 grid: ties everywhere
    cnt = rng.integers(0, K + 1, (B, nc)).astype(np.int32)
    cnt[1] = rng.integers(0, 20, nc)                                                 # this image stays below the cap
    want = np.stack([R.cap_counts(out[b], cnt[b], 200) for b in range(B)])
    assert want[0].sum() == 200 and want[1].sum() == cnt[1].sum() < 200
    assert np.array_equal(_cap(out, cnt, 200), want)


# ---- the matching, rule by rule

def test_empty_cells_and_truncation_to_100():
    nc, K = 3, 120
    many = [(1 + 0.25 * i, 2, 40 + 0.25 * i, 50, 1 - i / 128) for i in range(K)]
    gts = [(1, 2, 40, 50, 0), (100, 100, 180, 190, 1)]
    images = [({}, gts),                              # D = 0, G > 0
              ({0: many[:7], 2: many[:3]}, []),       # G = 0 (count), D > 0
              ({}, []),                               # both 0
              ({0: many[:101], 1: many}, gts)]        # cnt = 101 and cnt = K
    rec, _ = _check(_scene(images, nc, K, 2), nc)
    assert list(rec['ndt'][3]) == [100, 100, 0] and list(rec['ndt'][1]) == [7, 0, 3] and not rec['ndt'][[0, 2]].any()
    assert list(rec['ngt'][0, :, 0]) == [1, 1, 0] and not rec['ngt'][1:3].any()
    assert not rec['dtm'][1].any() and not rec['score'][2].any()
    # a batch with no ground-truth slots at all
    out, cnt, gb, gl, gc, shapes = _scene(images[1:3], nc, K, 0)
    assert gb.shape == (2, 0, 4)
    _check((out, cnt, gb, gl, gc, shapes), nc)


def test_64_ground_truths_in_one_cell():
    rng = np.random.default_rng(11)
    G, nc, K = 64, 2, 40
    xy = np.round(rng.uniform(0, 200, (G, 2)) * 4) / 4
    wh = np.round(rng.uniform(8, 90, (G, 2)) * 4) / 4
    gts = [(x, y, x + w, y + h, 0) for (x, y), (w, h) in zip(xy, wh)]
    jit = np.round(rng.normal(0, 3, (K, 4)) * 4) / 4
    dets = [(gts[i][0] + j[0], gts[i][1] + j[1], gts[i][2] + j[2], gts[i][3] + j[3], 1 - i / 64) for i, j in enumerate(jit)]
    rec, _ = _check(_scene([({0: dets, 1: dets[:5]}, gts)], nc, K, G, shapes=[(480, 640)]), nc)
    assert rec['ngt'][0, 0, 0] == 64 and rec['dtm'][0, 0].any()


def test_invalid_ground_truth_slots_are_skipped():
    nc = 2
    gts = [(10, 10, 60, 60, 0), (np.nan, 10, 60, 60, 0), (10, 10, 10, 60, 0), (10, 60, 60, 10, 0), (10, 10, 60, 60, 2),
           (10, 10, 60, 60, -1), (np.inf, 0, np.inf, 9, 0), (100, 100, 160, 160, 1), (0, 0, 50, 50, 0)]
    dets = {0: [(10, 10, 60, 60, .9)], 1: [(100, 100, 160, 160, .8)]}
    arrays = _scene([(dets, gts)], nc, 4, len(gts))
    arrays[4][0] = len(gts) - 1                 # the last slot lies past the count
    rec, _ = _check(arrays, nc)
    assert list(rec['ngt'][0, :, 0]) == [1, 1]
    assert _bits(rec['dtm'][0, 0, 0], 0) == 0x3ff and _bits(rec['dtm'][0, 1, 0], 0) == 0x3ff


def test_competition_ties_the_break_rule_and_area_ranges():
    nc, K = 5, 4
    images = [
        ({0: [(0, 0, 40, 40, .9), (0, 0, 40, 42, .8)],                  # class 0: two detections compete for one ground truth
          1: [(0, 0, 10, 10, .9), (0, 0, 20, 10, .8)],                  # class 1: equal IoU with two ground truths
          2: [(0, 0, 40, 40, .9)],                                      # class 2: the break rule at `small`
          3: [(50, 50, 52, 52, .9)],                                    # class 3: unmatched, outside medium and large
          4: []},
         [(0, 0, 40, 40, 0), (0, 0, 10, 20, 1), (0, 0, 20, 10, 1), (0, 0, 30, 30, 2), (0, 0, 40, 40, 2),
          (100, 100, 132, 132, 4), (100, 100, 196, 196, 4)])]            # class 4: areas exactly 1024 and 9216
    rec, _ = _check(_scene(images, nc, K, 7), nc)
    dtm, dtig = rec['dtm'][0], rec['dtig'][0]
    # the better-scoring detection takes the ground truth at every threshold, the second one is left without
    assert _bits(dtm[0, 0], 0) == 0x3ff and _bits(dtm[0, 1], 0) == 0
    # IoU 1/2 with both: the LATER ground truth (0, 0, 20, 10) is taken, so the second detection, which is that box, finds
    # only (0, 0, 10, 20) free at threshold .5: IoU 1/3, no match (from .55 on the first matches nothing and leaves it its box)
    assert _bits(dtm[1, 0], 0) == 1 and _bits(dtm[1, 1], 0) == 0x3fe
    # `small`: IoU 1 with the ignored 40 x 40 box, .5625 with the 30 x 30 one -- the walk stops at the non-ignored match
    # for thresholds .5 and .55, and reaches the ignored box from .6 on
    assert _bits(dtm[2, 0], 1) == 0x3ff and _bits(dtig[2, 0], 1) == 0x3fc
    assert _bits(dtig[3, 0], 0) == 0 and _bits(dtig[3, 0], 1) == 0 and _bits(dtig[3, 0], 2) == 0x3ff and _bits(dtig[3, 0], 3) == 0x3ff
    assert _bits(dtm[3, 0], 0) == 0
    # both ends of a range are inclusive: 1024 is small and medium, 9216 medium and large
    assert list(rec['ngt'][0, 4]) == [2, 1, 2, 1]


def test_per_image_original_shapes():
    nc, K = 2, 3
    dets = {0: [(30.25, 40.5, 90.75, 100.25, .9), (200, 10, 260.5, 80, .5)], 1: [(5, 5, 20.25, 17.75, .7)]}
    gts = [(31, 41, 92.5, 99, 0), (5.25, 5, 20, 18, 1), (150, 150, 170.5, 163.25, 1)]
    shapes = [(480, 640), (1440, 1920), (300, 300), (301, 299)]
    rec, _ = _check(_scene([(dets, gts)] * 4, nc, K, 3, shapes=shapes), nc)
    # the same boxes land in other area ranges at other frame sizes
    assert not np.array_equal(rec['ngt'][0], rec['ngt'][1]) and not np.array_equal(rec['dtig'][0], rec['dtig'][1])
    # a non-square network input
    _check(_scene([(dets, gts)] * 2, nc, K, 3, shapes=shapes[:2]), nc, size=(270, 300))


def _random_batch(rng, B, nc=9, K=200, Gmax=8):
    shapes = [(480, 640), (1440, 1920), (300, 300), (720, 960), (1080, 1920)]
    images, used = [], []
    for b in range(B):
        gts = []
        for _ in range(int(rng.integers(1, Gmax + 1))):
            w, h = rng.choice([6, 14, 30, 70, 150], 2) * rng.uniform(.7, 1.3, 2)
            x, y = rng.uniform(0, 300 - w), rng.uniform(0, 300 - h)
            gts.append(tuple(np.round(np.array([x, y, x + w, y + h]) * 4) / 4) + (int(rng.integers(0, nc - 1)),))   # never the last class
        dets = {}
        for c in range(nc):
            rows = []
            for g in gts:
                if g[4] == c:
                    for _ in range(int(rng.integers(0, 4))):
                        rows.append(np.array(g[:4]) + rng.normal(0, .08, 4) * (g[2] - g[0] + g[3] - g[1]))
            n_fp = int(rng.integers(0, 6)) + (25 if (b == 0 and c == 1) else 0)
            for _ in range(n_fp):
                w, h = rng.uniform(3, 200, 2)
                x, y = rng.uniform(0, 300 - w), rng.uniform(0, 300 - h)
                rows.append(np.array([x, y, x + w, y + h]))
            rows = [np.round(np.clip(r, 0, 300) * 4) / 4 for r in rows]
            scores = -np.sort(-np.round(rng.random(len(rows)) * 32) / 32)               # ties
            dets[c] = [tuple(r) + (s,) for r, s in zip(rows, scores)]
        images.append((dets, gts))
        used.append(shapes[int(rng.integers(0, len(shapes)))])
    return _scene(images, nc, K, Gmax, shapes=used)


@pytest.fixture(scope='module')
def random_batches():
    """Three batches (B = 3, 2, 3) with the restatement's record of each, computed once."""
    rng = np.random.default_rng(2024)
    batches = [_random_batch(rng, B) for B in (3, 2, 3)]
    recs = [R.record_of(*a, 300, 300, 200)[0] for a in batches]
    return batches, recs


def test_random_scenes_equal_the_restatement(random_batches):
    batches, recs = random_batches
    want = R.concat_records(recs)
    # the scenes must contain what they are here to test (from the restatement alone, before anything is compared)
    live = np.arange(100)[None, None, :] < want['ndt'][:, :, None]
    assert ((want['dtm'] & want['dtig']) != 0).any(), 'no matched detection that is ignored'
    assert ((~want['dtm'] & want['dtig'])[live] != 0).any(), 'no unmatched detection outside its area range'
    assert (want['ngt'][:, :, 0].sum(0) == 0).any(), 'no class without ground truth'
    assert want['ndt'].max() > 10, 'no cell with more than 10 detections'
    assert (want['ndt'].sum(1) > 0).all() and (want['ngt'][:, :, 1:].sum((0, 1)) > 0).all()

    from torchdet3d.evaluation import detection_eval as E
    ev = _evaluator(9, 10, max_per_img=200)
    # base > 0 from the second call on, and calls of different B append to one record
    for arrays in batches:
        ev.evaluate_detections(*[_dev(a) for a in arrays])
    assert ev.base == 8
    got = ev.record()
    _same(got, want)
    res = ev.finalize()
    assert res is ev.finalize() and res['images'] == 8
    p, r = R.accumulate(want)
    stats = R.summarize(p, r)
    assert np.abs(res['stats'] - stats).max() <= 1e-12
    assert np.array_equal(res['precision'], p) and np.array_equal(res['recall'], r)
    assert (stats[:3] > 0).all() and (stats[:3] < 1).all()
    assert res['bbox_mAP'] == float(f'{stats[0]:.3f}') and list(res['classwise']) == list(ev.classes)
    assert np.isnan(res['classwise'][ev.classes[8]])
    assert (E.summarize(*E.accumulate(*[got[k] for k in KEYS])) == res['stats']).all()
    # the record is full: 8 of 10 rows, 3 more do not fit
    with pytest.raises(ValueError, match='record is full'):
        ev.evaluate_detections(*[_dev(a) for a in batches[0]])
    # reset starts over; every slot of a row is rewritten, so nothing of the old rows shows
    ev.reset()
    ev.evaluate_detections(*[_dev(a) for a in batches[2]])
    _same(ev.record(), recs[2], 'after reset')


def test_two_runs_give_identical_bytes(random_batches):
    batches, _ = random_batches
    blocks = []
    for _ in range(2):
        ev = _evaluator(9, 3, max_per_img=200)
        ev._record.fill_(0xa5)                     # whatever the record held before must not matter either
        ev.evaluate_detections(*[_dev(a) for a in batches[0]])
        torch.cuda.synchronize()
        blocks.append(ev._record.cpu().numpy())
    used = np.zeros(len(blocks[0]), bool)
    for off, n, _, _ in ev._layout.values():
        used[off:off + n] = True
    assert np.array_equal(blocks[0][used], blocks[1][used])


# ---- arguments

def _native_args(B=1, nc=2, K=3, G=2, R_=4):
    from torchdet3d import _native as N
    from torchdet3d.evaluation import detection_eval as E
    t = dict(out=torch.zeros(B, nc, K, 6, device='cuda'), cnt=torch.zeros(B, nc, dtype=torch.int32, device='cuda'),
             gb=torch.zeros(B, max(G, 1), 4, device='cuda'), gl=torch.zeros(B, max(G, 1), dtype=torch.int32, device='cuda'),
             gc=torch.zeros(B, dtype=torch.int32, device='cuda'), sh=torch.full((B, 2), 300, dtype=torch.int32, device='cuda'),
             thr=_dev(E.make_iou_thresholds()), rng=_dev(E.make_area_ranges()),
             score=torch.zeros(R_, nc, 100, device='cuda'), dtm=torch.zeros(R_, nc, 100, dtype=torch.int64, device='cuda'),
             dtig=torch.zeros(R_, nc, 100, dtype=torch.int64, device='cuda'), ndt=torch.zeros(R_, nc, dtype=torch.int32, device='cuda'),
             ngt=torch.zeros(R_, nc, 4, dtype=torch.int32, device='cuda'), valid=torch.zeros(R_, dtype=torch.int32, device='cuda'))
    p = {k: N.ptr(v) for k, v in t.items()}
    args = [p['out'], p['cnt'], B, nc, K, p['gb'], p['gl'], p['gc'], G, p['sh'], 300, 300, p['thr'], p['rng'], 0, R_,
            p['score'], p['dtm'], p['dtig'], p['ndt'], p['ngt'], p['valid'], N.stream()]
    return t, args


def test_entry_points_check_their_arguments():
    from torchdet3d import _native as N
    lib = N.lib()
    keep, args = _native_args()
    assert lib.t3d_coco_match(*args) == 0

    def with_(i, v):
        a = list(args)
        a[i] = v
        return a
    assert lib.t3d_coco_match(*with_(8, 65)) == N.ERR_UNSUPPORTED                 # G > 64
    assert lib.t3d_coco_match(*with_(14, 4)) == N.ERR_ARG                          # base + B > R
    assert lib.t3d_coco_match(*with_(14, 3)) == 0
    assert lib.t3d_coco_match(*with_(14, -1)) == N.ERR_ARG
    for i in (0, 1, 5, 6, 7, 9, 12, 13, 16, 17, 18, 19, 20, 21):                   # NULL pointers
        assert lib.t3d_coco_match(*with_(i, None)) == N.ERR_ARG, i
    for i in (12, 13, 17, 18):                                                     # 8-byte sections 4 bytes off
        assert lib.t3d_coco_match(*with_(i, args[i] + 4)) == N.ERR_ARG, i
    assert lib.t3d_coco_match(*with_(0, args[0] + 2)) == N.ERR_ARG
    for i, v in ((2, -1), (3, 0), (4, 0), (8, -1), (10, 0), (11, -5)):
        assert lib.t3d_coco_match(*with_(i, v)) == N.ERR_ARG, (i, v)
    launches = N.launch_count()
    assert lib.t3d_coco_match(*with_(2, 0)) == 0 and N.launch_count() == launches  # B == 0: nothing launched
    res = torch.zeros(1, 2, dtype=torch.int32, device='cuda')
    cap = [args[0], args[1], 1, 2, 3, 5, N.ptr(res), N.stream()]
    assert lib.t3d_ssd_cap_per_image(*cap) == 0
    for i, v in ((0, None), (1, None), (6, None), (2, -1), (3, 0), (4, 0), (5, -1), (6, cap[6] + 1)):
        a = list(cap)
        a[i] = v
        assert lib.t3d_ssd_cap_per_image(*a) == N.ERR_ARG, (i, v)
    a = list(cap)
    a[3], a[4] = 9, 456                                                            # 4104 rows
    assert lib.t3d_ssd_cap_per_image(*a) == N.ERR_UNSUPPORTED
    a = list(cap)
    a[2] = 0
    launches = N.launch_count()
    assert lib.t3d_ssd_cap_per_image(*a) == 0 and N.launch_count() == launches
    torch.cuda.synchronize()
    del keep


def test_evaluator_checks_its_arguments():
    from torchdet3d.evaluation import DetectionEvaluator
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DetectionEvaluator(None, 4, device='cpu', num_classes=2, max_per_img=5)
    with pytest.raises(ValueError):
        DetectionEvaluator(None, 0, num_classes=2, max_per_img=5)
    ev = _evaluator(2, 4)
    arrays = _scene([({0: [(0, 0, 5, 5, .5)]}, [(0, 0, 5, 5, 0)])], 2, 3, 2)
    good = [_dev(a) for a in arrays]
    for i in range(6):
        bad = list(good)
        bad[i] = good[i].cpu()
        with pytest.raises(RuntimeError, match='must be a device tensor'):
            ev.evaluate_detections(*bad)
    for i, shape in ((0, (1, 3, 3, 6)), (0, (1, 2, 3, 5)), (1, (1, 3)), (2, (1, 2, 3)), (3, (1, 3)), (4, (2,)), (5, (1, 3))):
        bad = list(good)
        bad[i] = torch.zeros(shape, dtype=good[i].dtype, device='cuda')
        with pytest.raises(ValueError, match='shape|must be'):
            ev.evaluate_detections(*bad)
    big = _scene([({}, [])], 2, 3, 65)
    with pytest.raises(ValueError, match='G <= 64'):
        ev.evaluate_detections(*[_dev(a) for a in big])
    if torch.cuda.device_count() > 1:
        bad = list(good)
        bad[0] = good[0].to('cuda:1')
        with pytest.raises(ValueError, match='the evaluator on'):
            ev.evaluate_detections(*bad)
    with pytest.raises(RuntimeError, match='without a detector'):
        ev.evaluate(torch.zeros(1, 300, 300, 3, dtype=torch.uint8, device='cuda'), *good[2:])
    assert ev.base == 0
    ev.evaluate_detections(*good)
    assert ev.base == 1 and ev.finalize()['images'] == 1


# ---- the validation loop, end to end

TEST_PIPELINE = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(300, 300), flip=False,
         transforms=[dict(type='Resize', keep_ratio=False), dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
                     dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]),
]
TRAIN_PIPELINE = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion', brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18),
    dict(type='Albu', transforms=[dict(type='RandomRotate90and270', p=0.5)], update_pad_shape=False, skip_img_without_anno=True),
    dict(type='Expand', ratio_range=(1, 3)),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.1),
    dict(type='Resize', img_scale=(300, 300), keep_ratio=False),
    dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]


def _write_dataset(root, n=5):
    from PIL import Image
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    rng = np.random.default_rng(42)
    images, anns = [], []
    for i in range(n):
        h, w = int(rng.integers(60, 120)), int(rng.integers(80, 160))
        fn = f'images/{i:03d}.png'
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, fn))
        images.append(dict(id=i + 1, file_name=fn, width=w, height=h))
        for _ in range(int(rng.integers(1, 4))):
            x, y = float(rng.uniform(0, w * .5)), float(rng.uniform(0, h * .5))
            anns.append(dict(id=len(anns), image_id=i + 1, category_id=int(rng.integers(1, 10)), iscrowd=0,
                             bbox=[x, y, float(rng.uniform(8, w * .45)), float(rng.uniform(8, h * .45))]))
    for name in ('objectron_train.json', 'objectron_test.json'):
        with open(os.path.join(root, 'annotations', name), 'w') as f:
            json.dump(dict(images=images, annotations=anns, categories=[]), f)


def _stats_ok(res, images):
    assert res['images'] == images and res['stats'].shape == (12,)
    assert all(v == -1 or 0 <= v <= 1 for v in res['stats'])
    assert res['precision'].shape == (10, 101, 9, 4, 3) and res['recall'].shape == (10, 9, 4, 3)


def _val_by_hand(det, val):
    """The same epoch through `detect_device` + `evaluate_detections` batch by batch, and through the restatement."""
    from torchdet3d.evaluation import DetectionEvaluator
    ev, recs = DetectionEvaluator(det, 8), []
    for imgs, gb, gl, gc, shapes in val:
        out, cnt = det.detect_device(imgs)
        ev.evaluate_detections(out, cnt, gb, gl, gc, shapes, input_size=tuple(imgs.shape[1:3]))
        torch.cuda.synchronize()
        recs.append(R.record_of(*[t.cpu().numpy() for t in (out, cnt, gb, gl, gc, shapes)], 300, 300, det.max_per_img)[0])
    return ev, R.concat_records(recs)


def test_val_over_a_loader_untrained_and_after_two_training_steps(tmp_path):
    from torchdet3d.builders import build_detection_loader
    from torchdet3d.evaluation import DetectionEvaluator
    from torchdet3d.models.ssd import SSD300
    from torchdet3d.trainer.detection import DetectorTrainer
    root = str(tmp_path)
    _write_dataset(root)
    cfg = dict(input_size=300, train_pipeline=TRAIN_PIPELINE, test_pipeline=TEST_PIPELINE, seed=7,
               data=dict(samples_per_gpu=2, workers_per_gpu=0,
                         train=dict(type='RepeatDataset', times=1,
                                    dataset=dict(type='CocoDataset', classes=None, min_size=17, img_prefix=root,
                                                 ann_file=os.path.join(root, 'annotations/objectron_train.json'))),
                         val=dict(type='CocoDataset', img_prefix=root, test_mode=True,
                                  ann_file=os.path.join(root, 'annotations/objectron_test.json'))))
    train, val = build_detection_loader(cfg)
    det = SSD300(device='cuda:0', dtype=torch.bfloat16)
    ev = DetectionEvaluator(det, 8)
    res = ev.val(val)
    _stats_ok(res, 5)
    assert ev.base == 5 and [len(b[0]) for b in val] == [2, 2, 1]
    h = ev.record()
    print('untrained: detections per image', h['ndt'].sum(1), 'ground truths per image', h['ngt'][:, :, 0].sum(1), 'stats', res['stats'])
    assert (h['ndt'].sum(1) > 0).all() and (h['ngt'][:, :, 0].sum(1) > 0).all()        # the comparison below is not over nothing

    def check_against_the_restatement(res, ev):
        hand, want = _val_by_hand(det, val)
        _same(ev.record(), want)
        _same(hand.record(), want)
        stats = R.summarize(*R.accumulate(want))
        assert np.abs(res['stats'] - stats).max() <= 1e-12 and np.abs(hand.finalize()['stats'] - stats).max() <= 1e-12
    check_against_the_restatement(res, ev)

    trainer = DetectorTrainer(det)
    for batch, _ in zip(train, range(2)):
        trainer.train_step(*batch[:4], epoch=0)
    res2 = ev.val(val)                          # `val` resets the record and needs nothing switched on the detector
    _stats_ok(res2, 5)
    assert res2 is not res
    check_against_the_restatement(res2, ev)
