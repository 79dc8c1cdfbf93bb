"""CPU checks of the tracker: the numpy restatement (tests/tracker_ref.py, what the GPU tests hold csrc/track.hip to)
against goldens recorded from the reference's own IOUTracker (tests/golden/tracker.npz, tools/gen_tracker_golden.py), and
the host-side surface of torchdet3d.utils.IOUTracker that needs no device.

Bounds: boxes, ids, counts, num_tracks and last_global_id exact.  Keypoints 2e-6 absolute: they are O(1), the reference
takes a new track's first update and interpolated entries in float32 where the restatement (and the kernel) use float64 --
a few 2^-24 = 6e-8 per such step -- and the EMA damps earlier error by 0.7 per frame, so the sum stays under about 1e-6."""
import os

import numpy as np
import pytest

import tracker_ref as R
from conftest import GOLDEN

KP_TOL = 2e-6
SCENES = R.load_scenes(os.path.join(GOLDEN, 'tracker.npz'))


def test_golden_file_covers_the_parameter_sets():
    names = [s['name'] for s in SCENES]
    assert len(names) == 16 and len(set(names)) == 16
    for prefix in ('defaults/', 'demo/', 'demo_align/', 'tight/'):
        assert sum(n.startswith(prefix) for n in names) == 4
    assert all(len(s['frames']) == 48 for s in SCENES)
    assert any(len(b) == 0 for s in SCENES for b, _ in s['frames'])
    assert any((b[:, 2] == b[:, 0]).any() for s in SCENES for b, _ in s['frames'] if len(b))      # zero-area detections


@pytest.mark.parametrize('scene', SCENES, ids=[s['name'] for s in SCENES])
def test_restatement_matches_the_reference_goldens(scene):
    t = R.RefTracker(**scene['params'])
    for f, ((boxes, kps), (eb, ek, ei, nt, lg)) in enumerate(zip(scene['frames'], scene['expected'])):
        t.process(boxes, kps)
        ob, ok, oi = t.tracked()
        assert len(ob) == len(eb), f'frame {f}: {len(ob)} tracked objects, the reference has {len(eb)}'
        assert np.array_equal(ob, eb), f'frame {f}: boxes'
        assert np.array_equal(oi, ei), f'frame {f}: ids'
        assert t.num_tracks == nt and t.last_global_id == lg, f'frame {f}: num_tracks / last_global_id'
        if len(ek):
            assert np.abs(ok - ek).max() <= KP_TOL, f'frame {f}: keypoints {np.abs(ok - ek).max()}'


def test_assignment_solver_against_brute_force():
    import itertools
    rng = np.random.default_rng(0)
    for n, m in [(1, 1), (1, 4), (4, 1), (3, 3), (2, 5), (5, 2), (5, 6), (6, 6)]:
        for _ in range(5):
            c = rng.random((n, m)).astype(np.float32)
            r, k = R.solve_assignment(c)
            a = c.T if n > m else c
            best = min(a[np.arange(a.shape[0]), list(p)].astype(np.float64).sum()
                       for p in itertools.permutations(range(a.shape[1]), a.shape[0]))
            assert len(r) == min(n, m) and len(set(r)) == len(r) and len(set(k)) == len(k)
            assert abs(c[r, k].astype(np.float64).sum() - best) < 1e-12


def test_restatement_cap_drops_and_counts():
    boxes = np.array([[100 * i, 0, 100 * i + 50, 50] for i in range(6)], dtype=np.int32)
    kps = np.zeros((6, 18), np.float32)
    t = R.RefTracker(max_tracks=4)
    t.process(boxes, kps)
    assert t.num_tracks == 4 and t.dropped == 2 and t.last_global_id == 4
    assert np.array_equal(t.tracked()[0], boxes[:4])


def test_exported_from_utils_like_the_reference():
    from torchdet3d.utils import IOUTracker, TrackedObj
    assert TrackedObj._fields == ('rect', 'kp', 'label')
    import inspect
    names = list(inspect.signature(IOUTracker.__init__).parameters)[1:]
    assert tuple(names[:11]) == R.PARAM_NAMES
    assert names[11:] == ['device', 'streams', 'max_detections', 'max_tracks']
    defaults = {k: v.default for k, v in inspect.signature(IOUTracker.__init__).parameters.items() if k in R.DEFAULTS}
    assert defaults == R.DEFAULTS


@pytest.mark.parametrize('bad', [dict(time_window=0), dict(continue_time_thresh=0), dict(track_clear_thresh=0),
                                 dict(match_threshold=1.5), dict(match_threshold=-0.1), dict(track_detection_iou_thresh=2),
                                 dict(interpolate_time_thresh=-1), dict(detection_filter_speed=1.1),
                                 dict(keypoints_filter_speed=-1), dict(add_treshold=3), dict(no_updated_frames_treshold=-1),
                                 dict(no_updated_frames_treshold=2.0)], ids=lambda d: next(iter(d)))
def test_argument_assertions(bad):
    from torchdet3d.utils import IOUTracker
    with pytest.raises(AssertionError):
        IOUTracker(**bad)


def test_capacities_are_checked_without_a_device():
    from torchdet3d.utils import IOUTracker
    t = IOUTracker(max_detections=8)
    with pytest.raises(ValueError, match='max_detections'):
        t.process(None, [(0, 0, 10, 10, 0.9, 0)] * 9, [np.zeros(18, np.float32)] * 9)
    IOUTracker(max_detections=64, max_tracks=512)                   # 150 KiB of LDS: fits
    with pytest.raises(ValueError, match='LDS'):
        IOUTracker(max_detections=64, max_tracks=1024)              # the [64][1024] cost matrix alone is 256 KiB
    with pytest.raises(ValueError, match='LDS'):
        IOUTracker(max_detections=512, max_tracks=128)
    with pytest.raises(ValueError):
        IOUTracker(max_tracks=0)


def test_histories_are_refused_with_a_reason():
    from torchdet3d.utils import IOUTracker
    t = IOUTracker()
    for fn in (t.get_tracks, t.get_archived_tracks):
        with pytest.raises(NotImplementedError, match='not kept on the device'):
            fn()
