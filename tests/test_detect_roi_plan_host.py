"""CPU: `t3d_detect_roi_plan_host` (csrc/detect_roi.h run on the CPU) against numpy written here -- the source rectangle of a
drawn record in closed form, `dataloaders.jpeg.roi_mcus` and `plan_roi` for its MCU rectangle, segment run and block count, the
item, the rewritten record byte for byte -- over the records `t3d_detect_draw_host` makes for the cases of
tests/detect_draw_cases.py plus hand-made ones, on index rows of 4:2:0, 4:4:4 and gray files at seg_mcus 1, 2 and 3; the
rendering of the planned part with the rewritten record against the whole frame with the drawn one; records the augment
kernel refuses; the `data.decode_crop` key of `build_detection_loader` without a GPU."""
import numpy as np
import pytest

import detect_augment_ref as A
import detect_draw_cases as K
import detect_roi_cases as R
import jpeg_cases as C
from detect_roi_cases import B, INT_MAX, SAMPLINGS, SEG_MCUS, hand_made, index_rows

FLAGS = 127                      # include/t3d.h: every T3D_DET_* flag


# ---- the contract of include/t3d.h, restated ------------------------------------------------------------------------------------
def refused(r, src_bytes):
    """t3d_detect_augment_u8's rule for a bad record."""
    h, w, off = int(r['h']), int(r['w']), int(r['offset'])
    if h <= 0 or w <= 0 or off < 0 or off > src_bytes or h * w > (src_bytes - off) // 3:
        return True
    if int(r['turns']) not in (0, 1, 3) or int(r['flags']) & ~FLAGS:
        return True
    cw, ch = int(r['cx1']) - int(r['cx0']), int(r['cy1']) - int(r['cy0'])
    if cw <= 0 or ch <= 0 or cw > 1 << 24 or ch > 1 << 24:
        return True
    return sorted(int(p) for p in r['perm']) != [0, 1, 2]


def closed_form(r):
    """A good record -> ((x0, y0, x1, y1) in source pixels, (left, top) of the part in the canvas)."""
    h, w, t = int(r['h']), int(r['w']), int(r['turns'])
    left, top = int(r['left']), int(r['top'])
    rw, rh = (w, h) if t == 0 else (h, w)
    a0, a1 = max(int(r['cx0']) - left, 0), min(int(r['cx1']) - left, rw)
    b0, b1 = max(int(r['cy0']) - top, 0), min(int(r['cy1']) - top, rh)
    if a0 >= a1 or b0 >= b1:
        x0, y0, x1, y1 = 0, 0, 1, 1
    elif t == 0:
        x0, y0, x1, y1 = a0, b0, a1, b1
    elif t == 1:
        x0, y0, x1, y1 = w - b1, a0, w - b0, a1
    else:
        x0, y0, x1, y1 = b0, h - a1, b1, h - a0
    shift = {0: (x0, y0), 1: (y0, w - x1), 3: (h - y1, x0)}[t]
    return (x0, y0, x1, y1), (min(left + shift[0], INT_MAX), min(top + shift[1], INT_MAX))


def expected(rec, info, segs, item, src_bytes):
    """-> (record, item, rect [12], diag [2]) of one sample, from numpy and the package's host planner."""
    from torchdet3d.dataloaders import jpeg as J
    h, w = int(info['h']), int(info['w'])
    out = rec.copy()
    if refused(rec, src_bytes) or (int(rec['h']), int(rec['w'])) != (h, w):
        rect = (0, 0, w, h)
    else:
        rect, (left, top) = closed_form(rec)
        out['offset'], out['h'], out['w'], out['left'], out['top'] = item['out_offset'], rect[3] - rect[1], rect[2] - rect[0], left, top
    p = J.plan_roi(info, segs, *rect)
    assert p['mcus'] == J.roi_mcus(int(info['sampling']), h, w, *rect)
    it = item.copy()
    it['file_offset'], it['file_bytes'], it['reserved'] = int(item['file_offset']) + int(info['scan_offset']), info['scan_bytes'], 0
    it['seg_offset'] = int(item['seg_offset']) + p['seg_first']
    row = list(rect) + list(p['mcus']) + [p['seg_first'], p['seg_count'], 0, 0]
    return out, it, np.array(row, np.int32), np.array([(rect[2] - rect[0]) * (rect[3] - rect[1]), p['blocks']], np.int32)


# ---- records and index rows: tests/detect_roi_cases.py ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def drawn():
    return R.drawn()


def run(rec, info, file_bytes, src_bytes, sample=None):
    from torchdet3d.dataloaders.detection_arena import detect_roi_plan_host
    n = len(rec) if sample is None else len(sample)
    items = R.whole_items(n, info, file_bytes)
    return items, detect_roi_plan_host(rec, np.array([info] * n), items, src_bytes, sample)


# ---- the planner against numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_the_host_twin_equals_the_closed_form_and_plan_roi(drawn, sampling):
    seen = dict(turns=set(), empty=0, whole=0, part=0)
    for case, rec, src_bytes in drawn.values():
        for seg_mcus in SEG_MCUS:
            data, info, segs = index_rows(case['h'], case['w'], sampling, seg_mcus)
            items, (got_rec, got_items, got_rects, got_diag) = run(rec, info, len(data), src_bytes)
            for i in range(len(rec)):
                want = expected(rec[i], info, segs, items[i], src_bytes)
                where = (case['name'], sampling, seg_mcus, i)
                assert got_rec[i].tobytes() == want[0].tobytes(), where
                assert got_items[i].tobytes() == want[1].tobytes(), where
                assert np.array_equal(got_rects[i], want[2]) and np.array_equal(got_diag[i], want[3]), where
                # every field the contract does not name is the drawn record's
                for f in rec.dtype.names:
                    if f not in ('offset', 'h', 'w', 'left', 'top'):
                        assert got_rec[i][f].tobytes() == rec[i][f].tobytes(), (where, f)
                x0, y0, x1, y1 = (int(v) for v in got_rects[i, :4])
                seen['turns'].add(int(rec[i]['turns']))
                seen['empty'] += (x1 - x0, y1 - y0) == (1, 1)
                seen['whole'] += (x0, y0, x1, y1) == (0, 0, case['w'], case['h'])
                seen['part'] += 1 < (x1 - x0) * (y1 - y0) < case['h'] * case['w']
    assert seen['turns'] == {0, 1, 3} and min(seen['empty'], seen['whole'], seen['part']) > 50, seen


def test_the_hand_made_records_reach_the_corners_and_the_saturation():
    from torchdet3d.dataloaders.detection import DET_SAMPLE_DTYPE
    base = np.zeros(1, DET_SAMPLE_DTYPE)[0]
    base['perm'] = (0, 1, 2)
    h, w = 100, 130
    rec = hand_made(base, h, w, 0)
    rects = [closed_form(r)[0] for r in rec]
    for t in range(3):
        r = rects[R.PER_TURN * t:R.PER_TURN * (t + 1)]
        assert r[0] == (0, 0, w, h) and r[1] == r[2] == (0, 0, 1, 1)
        assert {r[5], r[6], r[7], r[8]} == {(0, 0, 1, 1), (w - 1, 0, w, 1), (0, h - 1, 1, h), (w - 1, h - 1, w, h)}
        assert r[10] == (0, 0, 1, 1)
    assert closed_form(rec[2 * R.PER_TURN - 1])[1][1] == INT_MAX and closed_form(rec[3 * R.PER_TURN - 1])[1][0] == INT_MAX       # top + w - 1, left + h - 1


# ---- the planned part renders as the whole frame does --------------------------------------------------------------------------
def render(frame, r, oh, ow):
    """t3d_detect_augment_u8's tap rule on one record, in numpy: the four taps of cv::resize in canvas coordinates, each the
    distorted source pixel under it or the fill; horizontal pass, vertical pass, every operation rounded on its own."""
    h, w, t = int(r['h']), int(r['w']), int(r['turns'])
    assert frame.shape == (h, w, 3)
    fl = int(r['flags'])
    img = A.distort(frame, dict(bright=r['delta'] if fl & 2 else None, contrast=r['alpha'] if fl & 4 else None, first=not fl & 8,
                                hsv=bool(fl & 16), sat=r['sat'] if fl & 32 else None, hue=r['hue'] if fl & 64 else None,
                                perm=tuple(int(p) for p in r['perm'])))
    rw, rh = (w, h) if t == 0 else (h, w)
    x0, x1, wx0, wx1 = A.coef(ow, int(r['cx1']) - int(r['cx0']), True)
    y0, y1, wy0, wy1 = A.coef(oh, int(r['cy1']) - int(r['cy0']), False)
    if fl & 1:
        x0, x1, wx0, wx1 = x0[::-1], x1[::-1], wx0[::-1], wx1[::-1]

    def tap(xs, ys):
        xr, yr = (int(r['cx0']) + xs - int(r['left']))[None, :], (int(r['cy0']) + ys - int(r['top']))[:, None]
        inside = (xr >= 0) & (xr < rw) & (yr >= 0) & (yr < rh)
        sx, sy = {0: (xr + 0 * yr, yr + 0 * xr), 1: (w - 1 - yr + 0 * xr, xr + 0 * yr), 3: (yr + 0 * xr, h - 1 - xr + 0 * yr)}[t]
        return np.where(inside[..., None], img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], A.F(0))
    a0, a1 = wx0[None, :, None], wx1[None, :, None]
    top = tap(x0, y0) * a0 + tap(x1, y0) * a1
    bot = tap(x0, y1) * a0 + tap(x1, y1) * a1
    out = top * wy0[:, None, None] + bot * wy1[:, None, None]
    assert out.dtype == np.float32
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


@pytest.mark.parametrize('size', [(24, 24), (300, 300)])
def test_the_part_with_the_rewritten_record_renders_as_the_frame_with_the_drawn_one(drawn, size):
    n, sizes = 0, set()
    for case, rec, src_bytes in drawn.values():
        if case['h'] > 100:
            continue
        data, info, _ = index_rows(case['h'], case['w'], '420', 2)
        frame = C.pillow(data)
        _, (new, _, rects, _) = run(rec, info, len(data), src_bytes)
        first = (case['h'], case['w']) not in sizes      # (the hand-made records are the same for every case of a size)
        sizes.add((case['h'], case['w']))
        for i in range(len(rec) if first else B):
            x0, y0, x1, y1 = (int(v) for v in rects[i, :4])
            want = render(frame, rec[i], *size)
            got = render(np.ascontiguousarray(frame[y0:y1, x0:x1]), new[i], *size)
            assert np.array_equal(got, want), (case['name'], i)
            n += 1
    assert n >= 200 and len(sizes) == 2


# ---- what the planner leaves alone ------------------------------------------------------------------------------------------------
def test_a_refused_record_a_missing_one_and_the_sample_table(drawn):
    case, rec, src_bytes = drawn['config/100x130/mid']
    data, info, segs = index_rows(100, 130, '420', 2)
    h, w = 100, 130
    bad = rec[:8].copy()
    bad['turns'][0] = 2
    bad['cx1'][1] = bad['cx0'][1]                       # an empty crop
    bad['perm'][2] = (0, 0, 2)
    bad['flags'][3] = 128
    bad['h'][4] = 99                                    # not the info's
    bad[5] = np.zeros(1, rec.dtype)[0]                  # the zero record t3d_detect_draw gives a bad sample
    bad['offset'][6] = src_bytes - 5                    # the frame does not fit src
    items, (new, got_items, rects, diag) = run(bad, info, len(data), src_bytes)
    whole = expected(bad[0], info, segs, items[0], src_bytes)
    assert tuple(whole[2][:4]) == (0, 0, w, h) and tuple(whole[2][4:10]) == (0, 0, 9, 7, 0, int(info['nseg']))
    for i in range(7):
        assert new[i].tobytes() == bad[i].tobytes(), i
        assert np.array_equal(rects[i], whole[2]) and np.array_equal(diag[i], whole[3]), i
        assert got_items[i].tobytes() == expected(bad[i], info, segs, items[i], src_bytes)[1].tobytes(), i
    assert new[7].tobytes() == expected(bad[7], info, segs, items[7], src_bytes)[0].tobytes()       # (the good one among them)
    # items in another order than their records, records without an item, an index outside the batch
    sample = np.array([9, 3, 40, -1, 0], np.int32)
    items, (new, got_items, rects, diag) = run(rec[:12], info, len(data), src_bytes, sample)
    for j, i in enumerate(sample):
        if 0 <= i < 12:
            want = expected(rec[i], info, segs, items[j], src_bytes)
            assert new[i].tobytes() == want[0].tobytes() and got_items[j].tobytes() == want[1].tobytes()
            assert np.array_equal(rects[j], want[2]) and np.array_equal(diag[j], want[3])
        else:
            assert tuple(rects[j, :4]) == (0, 0, w, h) and diag[j, 0] == h * w
    rest = [i for i in range(12) if i not in sample]
    assert new[rest].tobytes() == rec[rest].tobytes()
    # an info row the indexer would not write: whole-frame tables as they stand, no division by its zero, nothing rewritten
    broken = info.copy()
    broken['seg_mcus'] = 0
    from torchdet3d.dataloaders.detection_arena import detect_roi_plan_host
    new, _, rects, _ = detect_roi_plan_host(rec[:2], np.array([broken] * 2), items[:2], src_bytes)
    assert new.tobytes() == rec[:2].tobytes() and all(tuple(r[:10]) == (0, 0, w, h, 0, 0, 9, 7, 0, int(info['nseg'])) for r in rects)


def test_argument_errors():
    from torchdet3d import _native as N
    from torchdet3d.dataloaders import jpeg as J
    from torchdet3d.dataloaders.detection import DET_SAMPLE_DTYPE
    rec, infos, items = np.zeros(2, DET_SAMPLE_DTYPE), np.zeros(2, J.INFO_DTYPE), np.zeros(2, J.ITEM_DTYPE)
    out, rects, diag = np.zeros(2, J.ITEM_DTYPE), np.zeros((2, 12), np.int32), np.zeros((2, 2), np.int32)
    args = [rec.ctypes.data, 2, None, infos.ctypes.data, items.ctypes.data, 2, 100, out.ctypes.data, rects.ctypes.data, diag.ctypes.data,
            None]
    fn = N.lib().t3d_detect_roi_plan_host
    assert fn(*args) == 0
    for k, v in ((0, None), (3, None), (4, None), (7, None), (8, None), (9, None), (1, -1), (1, 65536), (5, -1), (5, 65536), (6, -1)):
        a = list(args)
        a[k] = v
        assert fn(*a) == N.ERR_ARG, (k, v)
    a = list(args)
    a[5] = 0
    a[0] = a[3] = a[4] = a[7] = a[8] = a[9] = None       # nothing to plan: nothing is looked at
    assert fn(*a) == 0


# ---- what the feature saves, as a statement about the inputs --------------------------------------------------------------------
def test_the_config_pipeline_asks_for_fewer_blocks_and_resize_flip_for_all(drawn):
    from torchdet3d.dataloaders import jpeg as J
    data, info, segs = index_rows(100, 130, '420', 1)
    frame_blocks = int(J.frame_blocks(np.array([info]))[0])
    for name, less in (('config/100x130/mid', True), ('resize_flip/100x130/mid', False)):
        case, rec, src_bytes = drawn[name]
        rec = rec[:B]
        want = sum(J.plan_roi(info, segs, *closed_form(r)[0])['blocks'] for r in rec)             # numpy alone
        assert (want < B * frame_blocks) if less else (want == B * frame_blocks), (name, want, B * frame_blocks)
        _, (_, _, _, diag) = run(rec, info, len(data), src_bytes)
        assert int(diag[:, 1].sum()) == want


# ---- the builder's key, without a GPU -------------------------------------------------------------------------------------------
def test_decode_crop_without_the_device_cache_raises(tmp_path):
    from torchdet3d.builders import build_detection_loader
    test = [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', img_scale=(300, 300), flip=False,
                                                 transforms=[dict(type='Resize', keep_ratio=False), dict(type='Collect', keys=['img'])])]
    root = str(tmp_path / 'nothing_here')
    data = dict(samples_per_gpu=2, workers_per_gpu=0, decode_crop=True, train=dict(img_prefix=root, ann_file=root + '/a.json'),
                val=dict(img_prefix=root, ann_file=root + '/a.json'))
    for extra in (dict(), dict(decode='device')):
        with pytest.raises(ValueError, match=r"data\.decode_crop.*data\.cache"):
            build_detection_loader(dict(input_size=300, train_pipeline=K.CONFIG, test_pipeline=test, seed=7, data=dict(data, **extra)))
