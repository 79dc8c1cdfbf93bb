"""CPU checks of the Objectron evaluation protocol: known answers of the plain-loop restatement
(tests/objectron_eval_ref.py), the host arithmetic of `ObjectronEvaluator.finalize` against it, the report text against a
golden file, and the two entry points' argument checks (their place in the C ABI: tests/test_abi.py).

A note on "every AP = 1" for prediction == ground truth: the lift is an eigenvector computation, so the exact prediction's
azimuth / polar / ADD / ADD-S come out as ~1e-10, not 0, and its IoU as 1 +- 1e-9.  At the one threshold per metric that EQUALS
the ideal value (0 for those four, 1.0 for IoU) the comparison is decided by that rounding, in any implementation; there the
test asks for the metric within 1e-6 of the ideal and an AP inside [0, 1].  Everywhere else -- 121 of 126 cells, the pixel
error's threshold 0 included, where the error is exactly 0 -- AP = 1 is asserted as it stands."""
import os

import numpy as np
import pytest
import torch

import objectron_eval_ref as R
from torchdet3d.evaluation import ObjectronEvaluator
from torchdet3d.evaluation import objectron_eval as E

def test_constants_and_thresholds_are_the_protocols():
    assert E.METRICS == R.METRICS
    assert (E.VIS, E.MAX_PIXEL, E.MAX_AZIMUTH, E.MAX_POLAR, E.MAX_DIST, E.NBINS) == (0.1, 0.1, 30.0, 20.0, 1.0, 21)
    thr = E.make_thresholds()
    assert thr.dtype == np.float64 and thr.shape == (6, 21)
    for i, m in enumerate(E.METRICS):
        assert np.array_equal(thr[i], R.THRESHOLDS[m])
    # the end points are the step-3 constants exactly: `metric <= thr` holds for an unmatched box at the last threshold
    assert thr[0, -1] == 0.1 and thr[1, -1] == 30.0 and thr[2, -1] == 20.0 and thr[3, -1] == 1.0 and thr[4, -1] == 1.0


def test_exact_prediction_is_a_perfect_score():
    rng = np.random.default_rng(3)
    rows = []
    for _ in range(3):
        inst = R.random_instance(rng)
        rows += R.evaluate_frames([R.make_frame([inst], [inst['kp2d']])])
    for r in rows:
        pixel, az, polar, iou, add, adds = r['metrics'][0]
        assert r['valid'] and r['matched'].tolist() == [0]
        assert pixel == 0.0
        assert az < 1e-6 and polar < 1e-6 and add < 1e-6 and adds < 1e-6
        assert abs(iou - 1.0) < 1e-6
    res = R.finalize(rows)
    assert res['matched'] == 3 and res['total_instances'] == 3 and res['error_2d'] == 0.0 and abs(res['iou_3d'] - 1) < 1e-6
    for m, name in enumerate(R.METRICS):
        for j in range(R.NBINS):
            on_the_ideal = (name == 'iou' and j == R.NBINS - 1) or (name not in ('iou', 'pixel') and j == 0)
            if on_the_ideal:
                assert 0.0 <= res['aps'][name][j] <= 1.0      # decided by rounding (docstring)
            else:
                assert res['aps'][name][j] == 1.0, (name, j)


def test_a_prediction_nearest_to_an_invisible_instance_gets_the_constants():
    rng = np.random.default_rng(4)
    hidden, seen = R.random_instance(rng, visibility=0.05), R.random_instance(rng)
    fr = R.make_frame([hidden, seen], [hidden['kp2d'] + 1e-3], plane=seen['plane'])
    row = R.evaluate_frames([fr])[0]
    assert row['valid'] and row['n'] == 2 and row['matched'].tolist() == [-1]
    assert row['metrics'][0].tolist() == [0.1, 30.0, 20.0, 0.0, 1.0, 1.0]
    for m, name in enumerate(R.METRICS):
        want = np.zeros(R.NBINS, np.int32)
        want[0 if name == 'iou' else -1] = 1
        assert np.array_equal(row['hit'][m], want), name
        assert np.array_equal(row['miss'][m], 1 - want), name
    assert row['sums'].tolist() == [0.0] * 5


def test_voc_average_precision_of_three_frames_by_hand():
    """hit / miss / instances = (1, 0, 2), (0, 1, 1), (1, 1, 1): tp = 1 1 2, fp = 0 1 2, recall = .25 .25 .5, precision = 1 .5 .5;
    padded and made monotone from the right: precision 1 1 .5 .5 0 over recall 0 .25 .25 .5 1; recall changes at indices 1, 3, 4:
    AP = .25 * 1 + .25 * .5 + .5 * 0 = .375."""
    assert R.average_precision([1, 0, 1], [0, 1, 1], 4) == pytest.approx(0.375, abs=1e-15)
    assert E.average_precision([1, 0, 1], [0, 1, 1], 4) == pytest.approx(0.375, abs=1e-15)
    assert E.average_precision([0, 0], [0, 0], 3) == 0.0 and E.average_precision([], [], 0) == 0.0
    assert E.average_precision([2, 1], [0, 0], 3) == pytest.approx(1.0, abs=1e-15)


def _synthetic_record(seed=0, rows=40):
    rng = np.random.default_rng(seed)
    valid = (rng.uniform(size=rows) > 0.25).astype(np.int32)
    n = rng.integers(1, 4, rows).astype(np.int32)
    npred = rng.integers(0, n + 1)                         # at most one prediction per instance: recall stays within 1
    hit = np.stack([rng.integers(0, k + 1, (6, 21)) for k in npred]).astype(np.int32)
    for m in range(6):                                     # cumulative over the thresholds, like real counts
        hit[:, m] = np.sort(hit[:, m], axis=1)[:, ::-1] if m == 3 else np.sort(hit[:, m], axis=1)
    miss = (npred[:, None, None] - hit).astype(np.int32)
    matched = np.minimum(npred, n)
    sums = np.stack([rng.uniform(0, 0.05, rows) * matched, rng.uniform(0, 1, rows) * matched, rng.uniform(0, 30, rows) * matched,
                     rng.uniform(0, 20, rows) * matched, matched.astype(np.float64)], 1)
    hit[valid == 0], miss[valid == 0], sums[valid == 0] = 0, 0, 0
    return valid, n, hit, miss, sums


def test_finalize_host_arithmetic_equals_the_restatement():
    valid, n, hit, miss, sums = _synthetic_record()
    assert 0 < valid.sum() < len(valid), 'the record has rows to drop'
    got = E.finalize_record(valid, n, hit, miss, sums)
    rows = [dict(valid=bool(valid[i]), n=int(n[i]), hit=hit[i], miss=miss[i], sums=sums[i]) for i in range(len(valid))]
    want = R.finalize(rows)
    for name in R.METRICS:
        assert np.abs(got['aps'][name] - want['aps'][name]).max() <= 1e-12, name
        assert np.array_equal(got['thresholds'][name], R.THRESHOLDS[name])
    for k in ('error_2d', 'iou_3d', 'azimuth', 'polar'):
        assert abs(got[k] - want[k]) <= 1e-12, k
    assert (got['matched'], got['total_instances'], got['frames']) == (want['matched'], want['total_instances'], want['frames'])
    inside = np.concatenate([(v > 0) & (v < 1) for v in want['aps'].values()])
    assert inside.mean() > 0.5, 'not a trivial record'
    empty = E.finalize_record(np.zeros(3, np.int32), n[:3], hit[:3] * 0, miss[:3] * 0, sums[:3] * 0)
    assert empty['matched'] == 0 and empty['error_2d'] == 0.0 and all((v == 0).all() for v in empty['aps'].values())


def test_report_text_equals_the_golden(golden_dir, tmp_path):
    valid, n, hit, miss, sums = _synthetic_record(seed=1, rows=25)
    text = E.format_report(E.finalize_record(valid, n, hit, miss, sums))
    want = open(os.path.join(golden_dir, 'objectron_report.txt')).read()
    assert text == want


def test_null_and_out_of_range_arguments_are_refused_before_any_launch():
    """Argument validation happens on the host, in front of the launch: no GPU is needed to see T3D_ERR_ARG."""
    from torchdet3d import _native as N
    lib, p = N.lib(), 4096            # (a non-null word; nothing is dereferenced on a refused call)
    good = [p] * 7 + [2, 3, 3, 1.0, 1.0, p, p, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 12, 13):
        bad = list(good)
        bad[i] = None
        assert lib.t3d_objectron_pairs(*bad) == -1, i
    for i in (7, 8, 9):
        for v in (0, -1):
            bad = list(good)
            bad[i] = v
            assert lib.t3d_objectron_pairs(*bad) == -1, (i, v)
    good = [p] * 8 + [2, 3, 3, 0, 8] + [p] * 5 + [None]
    for i in list(range(8)) + [13, 14, 15, 16, 17]:
        bad = list(good)
        bad[i] = None
        assert lib.t3d_objectron_hitmiss(*bad) == -1, i
    for i, v in ((8, 0), (9, 0), (10, -2), (11, -1), (11, 7), (12, 0), (12, 1)):       # F, P, G, base, record too small
        bad = list(good)
        bad[i] = v
        assert lib.t3d_objectron_hitmiss(*bad) == -1, (i, v)


def test_the_evaluator_is_exported_and_needs_a_gpu():
    import torchdet3d.evaluation as EV
    assert EV.ObjectronEvaluator is ObjectronEvaluator
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ObjectronEvaluator(4, 2, 2)
    with pytest.raises(RuntimeError):
        ObjectronEvaluator(4, 2, 2, device='cpu')
