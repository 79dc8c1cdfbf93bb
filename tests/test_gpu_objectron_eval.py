"""GPU: the Objectron evaluation stage (`t3d_objectron_pairs`, `t3d_objectron_hitmiss`, `ObjectronEvaluator`) against the
plain-loop numpy restatement of the protocol (tests/objectron_eval_ref.py) on one scene of F = 6 frames, P = G = 3:
  1. one object, exact prediction;  2. two objects, three noisy predictions, two on the same instance;  3. no prediction;
  4. every instance invisible or behind the camera (no row: `finalize` compacts);  5. a prediction nearest to an instance with
  visibility < VIS;  6. P_f = P, G_f = G.  Rows and slots past the counts hold nan, so reading one would show.
One integration case feeds `FramePipeline.process_device`'s own result to `evaluate_pipeline`.

Tolerances: per-slot IoU and lifted quantities 5e-6 (what test_gpu_geometry.py uses for random lifts against the oracle), pixel
error 1e-9; matched indices, valid, hit and miss exact; `finalize` against the restatement 1e-9.

Condition on the inputs, asserted on the REFERENCE values: every finite metric lies at least 1e-4 away from every threshold it is
compared with -- except the exact constants of an unmatched box, an IoU of exactly 0, and the exact-prediction frame's values at
the one threshold that equals their ideal: its IoU (1 +- 1e-9) against threshold 1.0, and its azimuth / polar / ADD / ADD-S
(~1e-10, the lift's rounding -- they cannot be 1e-4 away from threshold 0) against threshold 0.  Those cells of that frame's row
are checked by value only and left out of the exact hit / miss comparison; the frame's pixel error is exactly 0 on both sides and
stays in.  The average precision of those five (metric, threshold) cells is compared with the restatement's arithmetic fed the
device's own counts for that frame."""
import numpy as np
import pytest
import torch

import objectron_eval_ref as R

pytestmark = pytest.mark.gpu

try:                                                        # the frame pipeline's fixtures, for the integration case
    import test_gpu_frame_pipeline as TP
    from test_gpu_frame_pipeline import stages              # noqa: F401  (a fixture: pytest finds it in this module)
    TP_ERROR = None
except Exception as e:      # noqa: BLE001
    TP, TP_ERROR = None, e

SEED, P, G = 1, 3, 3
EXACT = 0                                                   # the exact-prediction frame
# (metric index, threshold index) decided by rounding for the exact frame
ROUNDING = [(3, R.NBINS - 1)] + [(m, 0) for m in (1, 2, 4, 5)]


def _dev(a):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items()}


def _evaluate(ev, d, frame_size=None, pred=None):
    return ev.evaluate(d['pred'] if pred is None else pred, d['pred_count'], d['kp2d'], d['kp3d'], d['vis'], d['gt_count'], d['planes'],
                       frame_size=frame_size)


@pytest.fixture(scope='module')
def scene():
    """The frames, the restatement's rows (computed once, never changed), the padded arrays and the device's results."""
    from torchdet3d.evaluation import ObjectronEvaluator
    frames = R.six_frame_scene(SEED)
    rows = R.evaluate_frames(frames)
    arrays = R.pack(frames, P, G, fill=np.nan)
    d = _dev(arrays)
    ev = ObjectronEvaluator(16, P, G)
    metrics, matched = _evaluate(ev, d)
    torch.cuda.synchronize()
    got = dict(metrics=metrics.cpu().numpy().copy(), matched=matched.cpu().numpy().copy(),
               **{k: v[:6].cpu().numpy().copy() for k, v in ev._r.items()})
    return dict(frames=frames, rows=rows, arrays=arrays, d=d, ev=ev, got=got)


def test_the_scene_is_what_the_docstring_says_and_keeps_its_distance_from_the_thresholds(scene):
    rows = scene['rows']
    assert [len(f['pred']) for f in scene['frames']] == [1, 3, 0, 1, 2, 3] and [r['n'] for r in rows] == [1, 2, 1, 2, 2, 3]
    assert [r['valid'] for r in rows] == [True, True, True, False, True, True]
    assert rows[1]['matched'].tolist() == [0, 1, 0] and rows[4]['matched'].tolist() == [-1, 1]
    assert sorted(rows[5]['matched'].tolist()) == [0, 1, 2]
    worst = np.inf
    for f, r in enumerate(rows):
        for vals, mi in zip(r['metrics'], r['matched']):
            if mi < 0:
                assert vals.tolist() == [0.1, 30.0, 20.0, 0.0, 1.0, 1.0]
                continue
            for m, name in enumerate(R.METRICS):
                if not np.isfinite(vals[m]) or (name == 'iou' and vals[m] == 0.0):
                    continue
                dist = np.abs(R.THRESHOLDS[name] - vals[m])
                if f == EXACT:
                    if name == 'pixel':
                        assert vals[m] == 0.0
                        dist = dist[1:]
                    else:
                        j = [t for mm, t in ROUNDING if mm == m][0]
                        assert dist[j] < 1e-6, (name, vals[m])
                        dist = np.delete(dist, j)
                worst = min(worst, dist.min())
    print(f'smallest distance of a reference metric from a threshold: {worst:.3e}')
    assert worst >= 1e-4


def test_per_slot_metrics_and_matches(scene):
    rows, got = scene['rows'], scene['got']
    worst = np.zeros(6)
    for f, r in enumerate(rows):
        n = len(r['matched'])
        assert np.array_equal(got['matched'][f, :n], r['matched']), f
        if n:
            worst = np.maximum(worst, np.abs(got['metrics'][f, :n] - r['metrics']).max(0))
    print('largest per-slot difference (pixel, azimuth, polar, iou, add, adds):', ' '.join(f'{w:.3e}' for w in worst))
    assert worst[0] <= 1e-9
    assert (worst[1:] <= 5e-6).all()


def test_valid_hit_and_miss_are_exactly_the_restatements(scene):
    rows, got = scene['rows'], scene['got']
    assert got['valid'].tolist() == [int(r['valid']) for r in rows]
    assert got['num_instances'].tolist() == [r['n'] for r in rows]
    for f, r in enumerate(rows):
        keep = np.ones((6, R.NBINS), bool)
        if f == EXACT:
            for m, j in ROUNDING:
                keep[m, j] = False
        assert np.array_equal(got['hit'][f][keep], r['hit'][keep]), f
        assert np.array_equal(got['miss'][f][keep], r['miss'][keep]), f
        assert np.array_equal(got['hit'][f] + got['miss'][f], np.full((6, R.NBINS), len(r['matched']) if r['valid'] else 0)), f
    assert not got['hit'][3].any() and not got['sums'][3].any(), 'the invalid frame contributes nothing'
    for f, r in enumerate(rows):
        assert got['sums'][f, 4] == r['sums'][4]
        assert np.abs(got['sums'][f, :4] - r['sums'][:4]).max() <= 3 * 5e-6


def test_finalize_equals_the_restatement(scene):
    rows, got, ev = scene['rows'], scene['got'], scene['ev']
    assert ev.base == 6
    res = ev.finalize()
    assert res is ev.finalize(), 'one read-back'
    mixed = [dict(r, hit=r['hit'].copy(), miss=r['miss'].copy()) for r in rows]
    for m, j in ROUNDING:
        mixed[EXACT]['hit'][m, j], mixed[EXACT]['miss'][m, j] = got['hit'][EXACT, m, j], got['miss'][EXACT, m, j]
    want = R.finalize(mixed)
    assert (res['frames'], res['matched'], res['total_instances']) == (5, want['matched'], want['total_instances']) == (5, 8, 9)
    for name in R.METRICS:
        err = np.abs(res['aps'][name] - want['aps'][name]).max()
        print(f'AP {name}: largest difference {err:.3e}')
        assert err <= 1e-9, name
        assert np.array_equal(res['thresholds'][name], R.THRESHOLDS[name])
    for k in ('error_2d', 'iou_3d', 'azimuth', 'polar'):
        print(f'mean {k}: device {res[k]!r} restatement {want[k]!r} difference {abs(res[k] - want[k]):.3e}')
    for k in ('error_2d', 'iou_3d', 'azimuth', 'polar'):
        assert abs(res[k] - want[k]) <= 1e-9, k


def test_a_second_call_appends_and_reset_starts_over(scene):
    from torchdet3d.evaluation import ObjectronEvaluator
    d, got = scene['d'], scene['got']
    ev = ObjectronEvaluator(8, P, G)
    _evaluate(ev, d)
    tail = {k: v[4:6].contiguous() for k, v in d.items()}
    _evaluate(ev, tail)
    assert ev.base == 8
    rec = {k: v.cpu().numpy() for k, v in ev._r.items()}
    for k in ('valid', 'num_instances', 'hit', 'miss', 'sums'):
        assert np.array_equal(rec[k][:6], got[k]), k
        assert np.array_equal(rec[k][6:8], got[k][4:6]), k
    assert ev.finalize()['frames'] == 7
    with pytest.raises(ValueError):
        _evaluate(ev, tail)                                  # the record is full
    assert ev.base == 8
    ev.reset()
    assert ev.base == 0
    _evaluate(ev, tail)
    res = ev.finalize()
    assert ev.base == 2 and res['frames'] == 2 and res['total_instances'] == 5


def test_finalize_waits_for_an_evaluate_on_another_stream(scene):
    from torchdet3d.evaluation import ObjectronEvaluator
    ev, side = ObjectronEvaluator(6, P, G), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _evaluate(ev, scene['d'])
    res, want = ev.finalize(), scene['ev'].finalize()          # read back on the default stream
    torch.cuda.current_stream().wait_stream(side)
    assert res['matched'] == want['matched'] and res['frames'] == want['frames']
    assert all(np.array_equal(res['aps'][m], want['aps'][m]) for m in R.METRICS)


def test_frame_pixels_with_a_frame_size_give_the_same_record(scene):
    """The scene in frame pixels with (W, H) = (480, 640) against the normalised path fed pixels * (1 / W, 1 / H) -- the
    kernel's own normalisation, so that both paths see the same keypoints to the last bit: the records are equal."""
    from torchdet3d.evaluation import ObjectronEvaluator
    d = scene['d']
    W, H = 480, 640
    pixels = d['pred'] * torch.tensor([W, H], dtype=torch.float64, device='cuda')
    normalised = pixels * torch.tensor([1.0 / W, 1.0 / H], dtype=torch.float64, device='cuda')
    a, b = ObjectronEvaluator(6, P, G), ObjectronEvaluator(6, P, G)
    ma, ia = _evaluate(a, d, frame_size=(W, H), pred=pixels.reshape(6, P, 18))
    mb, ib = _evaluate(b, d, pred=normalised)
    torch.cuda.synchronize()
    ra, rb = ({k: v.cpu().numpy() for k, v in e._r.items()} for e in (a, b))
    for k in ('valid', 'num_instances', 'hit', 'miss'):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.abs(ra['sums'] - rb['sums']).max() <= 1e-9
    worst = 0.0
    for f, n in enumerate(scene['arrays']['pred_count']):
        assert np.array_equal(ia[f, :n].cpu().numpy(), ib[f, :n].cpu().numpy()) and np.array_equal(ia[f, :n].cpu().numpy(), scene['rows'][f]['matched'])
        if n:
            worst = max(worst, np.abs(ma[f, :n].cpu().numpy() - mb[f, :n].cpu().numpy()).max())
            assert np.abs(ma[f, :n].cpu().numpy() - scene['got']['metrics'][f, :n]).max() <= 5e-6
    print(f'largest difference between the frame-pixel and the normalised path: {worst:.3e}')
    assert worst <= 1e-9


def test_bad_arguments_raise_and_nothing_is_appended(scene):
    from torchdet3d.evaluation import ObjectronEvaluator
    d = scene['d']
    ev = ObjectronEvaluator(8, P, G)
    with pytest.raises(RuntimeError):
        _evaluate(ev, dict(d, pred=d['pred'].cpu()))
    with pytest.raises(RuntimeError):
        _evaluate(ev, dict(d, planes=d['planes'].cpu()))
    with pytest.raises(ValueError):
        _evaluate(ev, dict(d, vis=d['vis'][:, :2].contiguous()))
    with pytest.raises(ValueError):
        _evaluate(ev, dict(d, pred_count=d['pred_count'][:5].contiguous()))
    with pytest.raises(ValueError):
        _evaluate(ObjectronEvaluator(8, 2, G), d)            # P above max_predictions
    with pytest.raises(ValueError):
        _evaluate(ObjectronEvaluator(4, P, G), d)            # more frames than rows
    assert ev.base == 0


def test_a_degenerate_prediction_completes_with_finite_or_missed_results(scene):
    """All nine keypoints on one point (the collapsed set test_gpu_geometry.py feeds the lift), and counts outside [0, P] /
    [0, G], which are clamped: ordinary input validation, every value either finite or a miss at every threshold."""
    from torchdet3d.evaluation import ObjectronEvaluator
    a = {k: v[:2].copy() for k, v in scene['arrays'].items()}
    a['pred'][0, 0] = 0.5
    a['pred'][1, :] = a['pred'][0, 0]
    a['pred_count'][1], a['gt_count'][1] = 7, 9               # clamped to P, G; the nan rows of the padding are then read
    a['kp2d'][1], a['kp3d'][1], a['vis'][1] = a['kp2d'][0], a['kp3d'][0], 1.0
    ev = ObjectronEvaluator(2, P, G)
    metrics, matched = _evaluate(ev, _dev(a))
    torch.cuda.synchronize()
    m, rec = metrics.cpu().numpy(), {k: v.cpu().numpy() for k, v in ev._r.items()}
    assert rec['valid'].tolist() == [1, 1] and rec['num_instances'].tolist() == [1, 3]
    assert (rec['hit'][0] + rec['miss'][0] == 1).all() and (rec['hit'][1] + rec['miss'][1] == 3).all()
    for f, n in ((0, 1), (1, 3)):
        for s in range(n):
            for k in range(6):
                v = m[f, s, k]
                if not np.isfinite(v):
                    assert rec['hit'][f, k].max() <= n - 1
    assert np.isfinite(m[:, :, 3][[0, 1, 1, 1], [0, 0, 1, 2]]).all() and (m[0, 0, 3] >= 0) and (m[0, 0, 3] <= 1 + 1e-9)
    assert np.isfinite(rec['sums']).all()
    res = ev.finalize()
    assert all(np.isfinite(v).all() for v in res['aps'].values()) and np.isfinite([res['error_2d'], res['iou_3d'], res['azimuth'], res['polar']]).all()


def test_frame_pipeline_results_feed_the_evaluator(request):
    """One integration case: the FramePipeline of test_gpu_frame_pipeline.py at its configuration (its `stages` fixture and
    `_tracker`, imported, not edited), frames until something is tracked, ground truth made from its own kp_frame: every
    tracked object matches itself with pixel error 0."""
    if TP is None:
        pytest.skip(f'the fixtures of test_gpu_frame_pipeline.py cannot be reused without editing it: {TP_ERROR!r}')
    from torchdet3d.evaluation import ObjectronEvaluator
    from torchdet3d.utils import FramePipeline
    det, reg, _, fd = request.getfixturevalue('stages')
    pipe = FramePipeline(det, reg, TP._tracker())
    S, T, H, W = TP.S, pipe.T, TP.H, TP.W
    for f in range(4):
        res = pipe.process_device(fd[f])
        count = res['count'].cpu().numpy()
        if count.sum() > 0:
            break
    assert count.sum() > 0, 'nothing tracked in four frames'
    kp = res['kp_frame'].cpu().numpy().reshape(S, T, 9, 2)
    for s in range(S):
        kp[s, count[s]:] = 0.0                                # rows past the count are stale
    kp2d = kp * np.array([1.0 / W, 1.0 / H])                  # the kernel's own normalisation
    rng = np.random.default_rng(0)
    box = R.random_instance(rng)
    kp3d = np.broadcast_to(box['kp3d'], (S, T, 9, 3)).copy()
    planes = np.broadcast_to(np.concatenate(box['plane']), (S, 6)).copy()
    ev = ObjectronEvaluator(4, T, T)
    gt = _dev(dict(kp2d=kp2d, kp3d=kp3d, vis=np.ones((S, T)), planes=planes))
    metrics, matched = ev.evaluate_pipeline(res, gt['kp2d'], gt['kp3d'], gt['vis'], res['count'], gt['planes'], frame_size=(W, H))
    torch.cuda.synchronize()
    m, mi = metrics.cpu().numpy(), matched.cpu().numpy()
    want_matched = 0
    for s in range(S):
        n = count[s]
        # every tracked object matches itself -- or an earlier one with the same corner keypoints: the first minimum wins
        first = [min(j for j in range(n) if np.array_equal(kp2d[s, i, 1:], kp2d[s, j, 1:])) for i in range(n)]
        assert mi[s, :n].tolist() == first
        assert (m[s, :n, 0] == 0.0).all()
        want_matched += n if R.num_instances(kp2d[s, :n], kp3d[s, :n], np.ones(n)) > 0 else 0      # a frame without a countable instance has no row
    out = ev.finalize()
    assert out['matched'] == want_matched and out['error_2d'] == 0.0
