"""CPU: the host half of the COCO bbox evaluation (torchdet3d/evaluation/detection_eval.py: thresholds, `accumulate`,
`summarize`, `report`) against the plain-loop restatement (tests/coco_eval_ref.py) on hand-checkable scenes, the tie order of
the merge sort, the maxDets slicing, the prefix property of the per-image cap against `SSD300.merge_classes`, and the
reported keys.  The records here come from the restatement's own `record_of`: no kernel runs."""
import numpy as np

import coco_eval_ref as R
from torchdet3d.evaluation import detection_eval as E

F = np.float32


def _batch(images, nc, K=4, G=2, size=300):
    """images: [(dets {class: [(x1, y1, x2, y2, score)]}, gts [(x1, y1, x2, y2, label)])] -> the arrays of a batch at
    ori_shape = input size (so coordinates are original-frame pixels as written)."""
    B = len(images)
    out, cnt = np.zeros((B, nc, K, 6), F), np.zeros((B, nc), np.int32)
    gb, gl, gc = np.zeros((B, G, 4), F), np.zeros((B, G), np.int32), np.zeros(B, np.int32)
    for b, (dets, gts) in enumerate(images):
        for c, rows in dets.items():
            cnt[b, c] = len(rows)
            for i, r in enumerate(rows):
                out[b, c, i, :5] = r
                out[b, c, i, 5] = c
        gc[b] = len(gts)
        for g, (x1, y1, x2, y2, lab) in enumerate(gts):
            gb[b, g], gl[b, g] = (x1, y1, x2, y2), lab
    shapes = np.full((B, 2), size, np.int32)
    return out, cnt, gb, gl, gc, shapes, size, size, 200


def _both(images, nc, **kw):
    rec, _ = R.record_of(*_batch(images, nc, **kw))
    want_p, want_r = R.accumulate(rec)
    got_p, got_r = E.accumulate(rec['score'], rec['dtm'], rec['dtig'], rec['ndt'], rec['ngt'], rec['valid'])
    assert got_p.shape == (10, 101, nc, 4, 3) and got_r.shape == (10, nc, 4, 3)
    assert np.array_equal(got_p, want_p) and np.array_equal(got_r, want_r)
    got_s, want_s = E.summarize(got_p, got_r), R.summarize(want_p, want_r)
    assert got_s.shape == (12,) and np.abs(got_s - want_s).max() <= 1e-12
    return rec, got_p, got_r, got_s


def test_the_parameters_are_cocoevals():
    assert np.array_equal(E.make_iou_thresholds(), np.linspace(.5, .95, 10)) and E.make_iou_thresholds().dtype == np.float64
    assert np.array_equal(E.make_rec_thresholds(), np.linspace(0, 1, 101))
    assert np.array_equal(E.make_area_ranges(), np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]))
    assert E.MAX_DETS == (1, 10, 100) and E.AREA_NAMES == ('all', 'small', 'medium', 'large')


def test_one_perfect_detection_gives_ap_1_and_a_class_without_ground_truth_stays_out():
    rec, p, r, s = _both([({0: [(10, 10, 60, 60, .9)], 1: [(0, 0, 5, 5, .8)]}, [(10, 10, 60, 60, 0)])], nc=2)
    assert abs(s[0] - 1) < 1e-12 and abs(s[1] - 1) < 1e-12 and abs(s[8] - 1) < 1e-12
    # class 1 has a detection and no ground truth: -1 everywhere, and the means above are over class 0 alone
    assert (p[:, :, 1] == -1).all() and (r[:, 1] == -1).all()
    # 50 x 50 = 2500: medium; small and large have no ground truth at all
    assert s[3] == -1 and abs(s[4] - 1) < 1e-12 and s[5] == -1


def test_iou_exactly_one_half_matches_the_first_threshold_only():
    rec, p, r, s = _both([({0: [(0, 0, 2, 1, .9)]}, [(0, 0, 1, 1, 0)])], nc=1)
    assert int(rec['dtm'][0, 0, 0]) & 0x3ff == 1                      # area range `all`: threshold .5 and no other
    assert (int(rec['dtm'][0, 0, 0]) >> 10) & 0x3ff == 1              # `small` (both areas are inside)
    assert abs(r[0, 0, 0, 2] - 1) < 1e-12 and (r[1:, 0, 0, 2] == 0).all()
    assert abs(s[0] - 0.1) < 1e-12 and abs(s[1] - 1) < 1e-12 and s[2] == 0


def test_identical_boxes_match_at_every_threshold():
    # IoU 1.0 against min(T, 1 - 1e-10)
    rec, p, r, s = _both([({0: [(3, 4, 50.25, 60.5, .5)]}, [(3, 4, 50.25, 60.5, 0)])], nc=1)
    assert int(rec['dtm'][0, 0, 0]) & 0x3ff == 0x3ff and int(rec['dtig'][0, 0, 0]) & 0x3ff == 0
    assert abs(s[0] - 1) < 1e-12


def test_a_false_positive_that_scores_above_the_true_positive_halves_the_precision():
    rec, p, r, s = _both([({0: [(200, 200, 250, 250, .9), (10, 10, 60, 60, .8)]}, [(10, 10, 60, 60, 0)])], nc=1)
    assert np.abs(p[:, :, 0, 0, 2] - 0.5).max() < 1e-12 and abs(s[0] - 0.5) < 1e-12
    assert (r[:, 0, 0, 0] == 0).all() and (r[:, 0, 0, 2] == 1).all()          # maxDets 1 sees the false positive alone


def test_equal_scores_keep_the_order_of_the_images():
    fp = ({0: [(200, 200, 250, 250, .5)]}, [])
    tp = ({0: [(10, 10, 60, 60, .5)]}, [(10, 10, 60, 60, 0)])
    _, _, _, s = _both([fp, tp], nc=1)
    assert abs(s[0] - 0.5) < 1e-12          # the false positive of the first image sorts first
    _, _, _, s = _both([tp, fp], nc=1)
    assert abs(s[0] - 1) < 1e-12


def test_max_dets_slices_the_matches_of_the_100_detection_matching():
    boxes = [(20 * i, 0, 20 * i + 16, 40, 0) for i in range(12)]
    dets = {0: [(b[0], b[1], b[2], b[3], 1 - i / 16) for i, b in enumerate(boxes)]}
    rec, p, r, s = _both([(dets, boxes)], nc=1, K=12, G=12)
    assert rec['ndt'][0, 0] == 12
    assert np.abs(r[:, 0, 0, 0] - 1 / 12).max() < 1e-12 and np.abs(r[:, 0, 0, 1] - 10 / 12).max() < 1e-12
    assert np.abs(r[:, 0, 0, 2] - 1).max() < 1e-12
    assert abs(s[6] - 1 / 12) < 1e-12 and abs(s[7] - 10 / 12) < 1e-12 and abs(s[8] - 1) < 1e-12


def test_the_cap_keeps_a_prefix_of_every_class_as_merge_classes_does():
    from torchdet3d.models.ssd import SSD300
    rng = np.random.default_rng(3)
    nc, K = 4, 6
    for trial in range(40):
        cnt = rng.integers(0, K + 1, nc).astype(np.int32)
        out = np.zeros((nc, K, 6), F)
        for c in range(nc):
            out[c, :, 4] = np.sort(rng.integers(1, 5, K).astype(F) / 8)[::-1]       # many ties, within and across classes
            out[c, :, 5] = c
            out[c, :, 0] = np.arange(K)                                             # the row's own index, to find it again
        for cap in (0, 1, 5, int(cnt.sum()), 1000):
            rows = SSD300.merge_classes(out.copy(), cnt, cap, input_size=1)
            kept = R.cap_counts(out, cnt, cap)
            assert kept.sum() == min(cap, cnt.sum()) == len(rows)
            assert np.array_equal(np.bincount(rows[:, 5].astype(int), minlength=nc), kept)
            want = sorted((c, i) for c in range(nc) for i in range(kept[c]))
            assert sorted((int(r[5]), int(r[0])) for r in rows) == want


def test_the_report_has_mmdets_keys_rounded_to_three_decimals():
    precision, recall = -np.ones((10, 101, 2, 4, 3)), -np.ones((10, 2, 4, 3))
    precision[:, :, 0, 0, 2] = 0.12345
    precision[0, :, 0, 0, 2] = 0.98765
    precision[:, :, 0, 2, 2] = 0.5
    recall[:, 0, 0, :] = 0.25
    res = E.report(precision, recall, ('cup', 'shoe'), 7)
    ap = (9 * 0.12345 + 0.98765) / 10
    assert res['bbox_mAP'] == float(f'{ap:.3f}') == 0.21 and res['bbox_mAP_50'] == 0.988 and res['bbox_mAP_75'] == 0.123
    assert res['bbox_mAP_s'] == -1.0 and res['bbox_mAP_m'] == 0.5 and res['bbox_mAP_l'] == -1.0
    assert res['bbox_mAP_copypaste'] == '0.210 0.988 0.123 -1.000 0.500 -1.000'
    assert abs(res['stats'][0] - ap) < 1e-12 and res['stats'].shape == (12,) and abs(res['stats'][8] - 0.25) < 1e-12
    assert abs(res['classwise']['cup'] - ap) < 1e-12 and np.isnan(res['classwise']['shoe'])
    assert res['images'] == 7 and res['precision'] is precision and res['recall'] is recall
    assert set(res) == {'bbox_mAP', 'bbox_mAP_50', 'bbox_mAP_75', 'bbox_mAP_s', 'bbox_mAP_m', 'bbox_mAP_l',
                        'bbox_mAP_copypaste', 'stats', 'precision', 'recall', 'classwise', 'images'}
