"""GPU: the joined frame pipeline (torchdet3d/utils/pipeline.py) and its three joint kernels (csrc/pipeline.hip).

The kernels are held to the host code they replace -- `SSD300.merge_classes` + `Detector._decode_detections`,
`numpy.argmax` + a gather, `Regressor.transform_kp` -- exactly: integers equal, floats bit-equal.  The joined chain is held to
the same stage objects driven by hand through the host at the SAME batch sizes (bit-equal: same kernels, same shapes), to
the per-frame public API (exact integers; keypoints within 1e-4, the project's keypoint bound between engines that run at
different batch sizes), and to itself replayed from a recorded plan (bit-equal)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---- 1. t3d_ssd_select_rects -------------------------------------------------------------------------------------------------
def _select(out, cnt, max_per_img, conf, H, W, ratio, D):
    from torchdet3d import _native as N
    F, nc, K = out.shape[:3]
    o, c = torch.from_numpy(out).cuda(), torch.from_numpy(cnt).cuda()
    res = dict(rects=torch.full((F, D, 4), 77, dtype=torch.int32, device='cuda'),
               crop_rects=torch.full((F * D, 4), 77, dtype=torch.int32, device='cuda'),
               scores=torch.full((F, D), 77.0, device='cuda'), det_labels=torch.full((F, D), 77, dtype=torch.int32, device='cuda'),
               counts=torch.full((F,), 77, dtype=torch.int32, device='cuda'), overflow=torch.full((F,), 77, dtype=torch.int32, device='cuda'))
    N.call('t3d_ssd_select_rects', N.ptr(o), N.ptr(c), F, nc, K, max_per_img, 300.0, float(conf), H, W, float(ratio[0]),
           float(ratio[1]), D, N.ptr(res['rects']), N.ptr(res['crop_rects']), N.ptr(res['scores']), N.ptr(res['det_labels']),
           N.ptr(res['counts']), N.ptr(res['overflow']), N.stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _select_ref(out, cnt, max_per_img, conf, H, W, ratio, D):
    """The product's host code: the merge helper, then Detector._decode_detections(...)[:D]."""
    from torchdet3d.models.ssd import SSD300
    from torchdet3d.utils import Detector
    det = Detector(types.SimpleNamespace(device='cuda'), conf=conf)
    det.expand_ratio = ratio
    F = out.shape[0]
    ref = dict(rects=np.zeros((F, D, 4), np.int32), crop_rects=np.zeros((F * D, 4), np.int32), scores=np.zeros((F, D), np.float32),
               det_labels=np.zeros((F, D), np.int32), counts=np.zeros(F, np.int32), overflow=np.zeros(F, np.int32))
    for f in range(F):
        lst = det._decode_detections(SSD300.merge_classes(out[f], cnt[f], max_per_img), (H, W))
        ref['overflow'][f] = max(len(lst) - D, 0)
        lst = lst[:D]
        ref['counts'][f] = len(lst)
        for j, (l, t, r, b, s, lab) in enumerate(lst):
            ref['rects'][f, j] = (l, t, r, b)
            ref['scores'][f, j] = np.float32(s)
            ref['det_labels'][f, j] = lab
            ref['crop_rects'][f * D + j] = (np.clip(l, 0, W), np.clip(t, 0, H) + f * H, np.clip(r, 0, W), np.clip(b, 0, H) + f * H)
    return ref


def _same(got, ref):
    for k in ref:
        if ref[k].dtype == np.float32:
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k          # bit-equal
        else:
            assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


CONF = 0.4


def _synthetic():
    """F = 3, nc = 3, K = 8.  Frame 0: 21 candidates (> max_per_img = 10), more than D = 4 survivors, equal scores across the
    classes, equal tops, coordinates below 0 and above 1.  Frame 1: three candidates, one exactly at float32(conf).  Frame 2:
    none.  Rows past the counts hold garbage that must not be read."""
    rng = np.random.default_rng(11)
    F, nc, K = 3, 3, 8
    out = np.zeros((F, nc, K, 6), np.float32)
    out[..., 0] = rng.uniform(-20, 250, (F, nc, K))
    out[..., 1] = rng.uniform(-20, 250, (F, nc, K))
    out[..., 2] = out[..., 0] + rng.uniform(5, 120, (F, nc, K))
    out[..., 3] = out[..., 1] + rng.uniform(5, 120, (F, nc, K))
    out[..., 4] = rng.uniform(0.05, 0.95, (F, nc, K))
    out[..., 5] = np.arange(nc)[None, :, None]
    cnt = np.array([[8, 7, 6], [2, 0, 1], [0, 0, 0]], np.int32)
    out[0, 0, 0, 4] = out[0, 1, 0, 4] = out[0, 2, 0, 4] = 0.93        # equal scores across classes
    out[0, 0, 1, 4] = out[0, 2, 1, 4] = 0.91
    out[0, 0, 0, 1] = out[0, 1, 0, 1] = out[0, 2, 1, 1] = 262.0        # equal tops, the largest: among the rows that go on
    out[0, 0, 0, 3] = out[0, 1, 0, 3] = out[0, 2, 1, 3] = 292.0        # (equal heights: the expanded tops stay equal)
    out[0, 2, 0, 1] = -7.5                                             # top below 0 ...
    out[0, 0, 1, 1] = 0.0                                              # ... ties with a top of exactly 0
    out[0, 1, 0, 2] = 330.0                                            # right above 1
    out[0, 0, 0, 0] = -12.0                                            # left below 0
    out[1, 0, 0, 4], out[1, 0, 1, 4], out[1, 2, 0, 4] = 0.9, np.float32(CONF), 0.41
    assert out[1, 0, 1, 4] == np.float32(CONF) and not out[1, 0, 1, 4] > np.float32(CONF)
    return out, cnt


@pytest.mark.parametrize('ratio', [(1., 1.), (1.2, 1.1)])
@pytest.mark.parametrize('H,W', [(37, 53), (1080, 1920)])
def test_select_rects_is_the_host_code(H, W, ratio):
    out, cnt = _synthetic()
    ref = _select_ref(out, cnt, 10, CONF, H, W, ratio, 4)
    assert ref['overflow'][0] > 0 and ref['counts'].tolist() == [4, 2, 0]
    assert len(set(ref['rects'][0, :, 1].tolist())) < 4, 'the fixture has equal tops among the rows that go on'
    _same(_select(out, cnt, 10, CONF, H, W, ratio, 4), ref)


def test_select_rects_at_the_detectors_worst_case():
    """nc x K = 9 x 200 = 1800 candidates in one frame (and a sparse second frame), scores on a coarse grid so that the
    stable order decides among many equal scores and equal tops."""
    rng = np.random.default_rng(5)
    F, nc, K = 2, 9, 200
    out = np.zeros((F, nc, K, 6), np.float32)
    out[..., 0] = rng.uniform(-20, 250, (F, nc, K))
    out[..., 1] = np.round(rng.uniform(-20, 250, (F, nc, K)) / 4) * 4
    out[..., 2] = out[..., 0] + rng.uniform(5, 120, (F, nc, K))
    out[..., 3] = out[..., 1] + rng.uniform(5, 120, (F, nc, K))
    out[..., 4] = np.round(rng.uniform(0.05, 0.95, (F, nc, K)) * 64) / 64
    out[..., 5] = np.arange(nc)[None, :, None]
    cnt = np.stack([np.full(nc, K), rng.integers(0, 3, nc)]).astype(np.int32)
    ref = _select_ref(out, cnt, 200, 0.5, 1080, 1920, (1.2, 1.1), 64)
    assert ref['counts'][0] == 64 and ref['overflow'][0] > 0
    _same(_select(out, cnt, 200, 0.5, 1080, 1920, (1.2, 1.1), 64), ref)


# ---- 2. t3d_head_select --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [9, 1, None])
def test_head_select_is_argmax_and_gather(C):
    from torchdet3d import _native as N
    rng = np.random.default_rng(2)
    n = 5
    kp_all = rng.standard_normal((9, n, 18)).astype(np.float32)
    logits = None
    if C is not None:
        logits = rng.standard_normal((n, C)).astype(np.float32)
        if C > 1:
            logits[3, 6] = logits[3, 2] = logits[3].max() + 1.0          # a tie: the lowest index wins
            logits[4, 8] = logits[4].max() + 1.0
    want = np.argmax(logits, 1) if C else np.zeros(n, np.int64)
    if C == 9:
        assert want[3] == 2 and want[4] == 8
    kd = torch.from_numpy(kp_all).cuda()
    ld = torch.from_numpy(logits).cuda() if C else None
    labels = torch.full((n,), 77, dtype=torch.int32, device='cuda')
    kp = torch.full((n, 18), 77.0, device='cuda')
    N.call('t3d_head_select', N.ptr(kd), N.ptr(ld), n, 9, C or 0, N.ptr(labels), N.ptr(kp), N.stream())
    assert np.array_equal(labels.cpu().numpy(), want.astype(np.int32))
    assert np.array_equal(kp.cpu().numpy(), kp_all[want, np.arange(n)])


# ---- 3. t3d_track_kp_to_frame --------------------------------------------------------------------------------------------------
def test_track_kp_to_frame_is_transform_kp():
    from torchdet3d import _native as N
    from torchdet3d.utils import Regressor
    rng = np.random.default_rng(3)
    S, T = 2, 8
    count = np.array([0, 5], np.int32)
    x0, y0 = rng.integers(-30, 1500, (S, T)), rng.integers(-30, 900, (S, T))
    boxes = np.stack([x0, y0, x0 + rng.integers(0, 700, (S, T)), y0 + rng.integers(0, 700, (S, T))], -1).astype(np.int32)
    kp = rng.uniform(-0.2, 1.2, (S, T, 18))                            # float64
    out = torch.full((S, T, 18), -5.0, dtype=torch.float64, device='cuda')
    cd, bd, kd = torch.from_numpy(count).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(kp).cuda()
    N.call('t3d_track_kp_to_frame', N.ptr(cd), N.ptr(bd), N.ptr(kd), N.ptr(out), S, T, N.stream())
    got = out.cpu().numpy()
    for s in range(S):
        for t in range(T):
            if t < count[s]:
                want = Regressor.transform_kp(np.array(tuple(kp[s, t])).reshape(9, 2), tuple(boxes[s, t].tolist()))
                assert np.array_equal(got[s, t].view(np.uint64), want.reshape(18).view(np.uint64)), (s, t)
            else:
                assert (got[s, t] == -5.0).all(), 'rows past the count are left as they were'


# ---- 4.-7. the joined chain ------------------------------------------------------------------------------------------------------
S, D, H, W = 2, 8, 120, 160
TRACK = dict(time_window=2, continue_time_thresh=2, track_clear_thresh=3)


@pytest.fixture(scope='module')
def stages():
    """Seeded SSD300 (bf16) + mobilenetv2 regressor on 96 x 96 crops, 8 frames of S = 2 cameras, and the confidence midway
    between the 5th and 6th best score of camera 0's first frame."""
    from oracle.weights import make_state_dict
    from test_gpu_two_stage import _ssd_pair
    from test_host_logic import _cfg
    from torchdet3d.builders import build_model
    from torchdet3d.utils import Detector, Regressor
    m, _, _, _ = _ssd_pair(torch.bfloat16)
    cfg = _cfg('mobilenetv2')
    cfg.model.storage_dtype = 'bf16'
    model = build_model(cfg, export_mode=True).to('cuda')
    model.load_state_dict(make_state_dict('mobilenetv2', 9))         # trained-looking weights: the outputs follow the crops
    reg = Regressor(model, (96, 96))
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (8, S, H, W, 3), dtype=np.uint8)
    det = Detector(m, conf=0.0)
    img, _ = det._enqueue(frames[0, 0])
    sc = np.sort(m.detect(img)[0][:, 4])[::-1]
    assert len(sc) >= 6 and sc[4] > sc[5]
    det.confidence = float((np.float64(sc[4]) + np.float64(sc[5])) / 2)
    return det, reg, frames, torch.from_numpy(frames).cuda()


def _tracker(streams=S):
    from torchdet3d.utils import IOUTracker
    return IOUTracker(**TRACK, device='cuda', streams=streams, max_detections=D, max_tracks=16)


def _snap(res):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().copy() for k, v in res.items()}
    for s in range(out['count'].shape[0]):                            # rows past the tracker's count are stale
        n = out['count'][s]
        for k in ('boxes', 'track_kp', 'ids', 'kp_frame'):
            out[k][s, n:] = 0
    return out


def _hand(det, reg, tr, fd):
    """One frame of every camera through the host, with the stage objects themselves: detect -> _decode_detections ->
    rectangles padded to D, Regressor.regress on the stacked frames, process_batch_device, transform_kp."""
    from torchdet3d.utils import Regressor
    Sn, Hn, Wn = fd.shape[:3]
    lists = det.get_detections_batch(fd)
    out = dict(counts=np.zeros(Sn, np.int32), rects=np.zeros((Sn, D, 4), np.int32), scores=np.zeros((Sn, D), np.float32),
               det_labels=np.zeros((Sn, D), np.int32), overflow=np.zeros(Sn, np.int32))
    crop = np.zeros((Sn * D, 4), np.int32)
    for s, lst in enumerate(lists):
        out['overflow'][s] = max(len(lst) - D, 0)
        lst = lst[:D]
        out['counts'][s] = len(lst)
        for j, (l, t, r, b, sc, lab) in enumerate(lst):
            out['rects'][s, j], out['scores'][s, j], out['det_labels'][s, j] = (l, t, r, b), np.float32(sc), lab
            crop[s * D + j] = (np.clip(l, 0, Wn), np.clip(t, 0, Hn) + s * Hn, np.clip(r, 0, Wn), np.clip(b, 0, Hn) + s * Hn)
    kp, labels = reg.regress(fd.reshape(Sn * Hn, Wn, 3), torch.from_numpy(crop).cuda())
    tr.process_batch_device(torch.from_numpy(out['rects']).cuda(), kp.reshape(Sn, D, 18).contiguous(),
                            torch.from_numpy(out['counts']).cuda())
    torch.cuda.synchronize()
    t = {k: v.cpu().numpy().copy() for k, v in tr.tracked_device().items()}
    out.update(labels=labels.cpu().numpy().astype(np.int32).reshape(Sn, D), kp=kp.cpu().numpy().reshape(Sn, D, 18),
               count=t['count'], scalars=t['scalars'], boxes=t['boxes'], ids=t['ids'], track_kp=t['kp'],
               kp_frame=np.zeros_like(t['kp']))
    for s in range(Sn):
        n = t['count'][s]
        for k in ('boxes', 'track_kp', 'ids'):
            out[k][s, n:] = 0
        for i in range(n):
            out['kp_frame'][s, i] = Regressor.transform_kp(np.array(tuple(t['kp'][s, i])).reshape(9, 2),
                                                           tuple(t['boxes'][s, i].tolist())).reshape(18)
    return out


def _bit_equal(got, want, what):
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k)


def test_joined_chain_equals_the_stages_driven_by_hand(stages, monkeypatch):
    from torchdet3d.utils import FramePipeline
    det, reg, _, fd = stages
    monkeypatch.setenv('T3D_STEP_PLAN', '0')
    pipe, lone = FramePipeline(det, reg, _tracker()), _tracker()
    seen = 0
    for f in range(6):
        got = _snap(pipe.process_device(fd[f]))
        want = _hand(det, reg, lone, fd[f])
        _bit_equal(got, want, f)
        seen += int(want['counts'].sum())
    assert pipe.replays == 0 and seen > 0
    assert want['count'].sum() > 0 and (want['ids'] >= 0).any(), 'tracks live long enough to carry ids'


def test_joined_chain_against_the_per_frame_public_api(stages, monkeypatch):
    """Detector.get_detections -> Regressor.get_detections -> IOUTracker.process -> get_tracked_objects -> transform_kp per
    camera, one frame at a time (the regressor then runs at the batch size of each frame's own count)."""
    from torchdet3d.utils import FramePipeline, Regressor
    det, reg, frames, fd = stages
    monkeypatch.setenv('T3D_STEP_PLAN', '0')
    pipe, solo = FramePipeline(det, reg, _tracker()), [_tracker(1) for _ in range(S)]
    compared, worst_kp, worst_pix = 0, 0.0, 0.0
    for f in range(4):
        got = _snap(pipe.process_device(fd[f]))
        for s in range(S):
            dets = det.get_detections(frames[f, s])[:D]
            n = len(dets)
            assert got['counts'][s] == n
            assert got['rects'][s, :n].tolist() == [list(d[:4]) for d in dets]
            assert got['det_labels'][s, :n].tolist() == [d[5] for d in dets]
            if n:
                # the host path's class logits: a top-two gap of 1e-3 keeps the arg-max out of reach of batch-size effects
                rects = torch.tensor([d[:4] for d in dets], dtype=torch.int32, device='cuda')
                _, logits = reg.model.forward_to_onnx(reg.crop_resize(fd[f, s], rects))
                top2 = torch.topk(logits, 2, dim=1).values
                gap = (top2[:, 0] - top2[:, 1]).min().item()
                print(f'frame {f} camera {s}: {n} detections, smallest top-two logit gap {gap:.3e}')
                assert gap >= 1e-3
            outs = reg.get_detections(frames[f, s], dets)
            assert got['labels'][s, :n].tolist() == [o[1] for o in outs]
            for i, (kp, _) in enumerate(outs):
                err = np.abs(got['kp'][s, i] - kp.reshape(18)).max()
                worst_kp = max(worst_kp, err)
                assert err <= 1e-4, (f, s, i, err)
                compared += 1
            solo[s].process(frames[f, s], dets, [o[0].reshape(-1) for o in outs])
            objs = solo[s].get_tracked_objects()
            assert got['count'][s] == len(objs)
            assert got['boxes'][s, :len(objs)].tolist() == [list(o.rect) for o in objs]
            assert [f'ID {i}' for i in got['ids'][s, :len(objs)]] == [o.label for o in objs]
            for i, o in enumerate(objs):
                pix = Regressor.transform_kp(np.array(o.kp).reshape(9, 2), o.rect[:4]).reshape(18)
                err = np.abs(got['kp_frame'][s, i] - pix).max()
                worst_pix = max(worst_pix, err)
                assert err <= 1e-4 * max(H, W), (f, s, i, err)
    print(f'{compared} detections compared: crop-normalised keypoints differ by at most {worst_kp:.3e}, frame pixels by {worst_pix:.3e}')
    assert compared > 0


def test_replayed_frames_are_bit_equal_and_follow_a_change_of_frame_size(stages, monkeypatch):
    from torchdet3d.utils import FramePipeline
    det, reg, _, fd = stages
    monkeypatch.setenv('T3D_STEP_PLAN', '0')
    direct = FramePipeline(det, reg, _tracker())
    monkeypatch.delenv('T3D_STEP_PLAN')
    replayed = FramePipeline(det, reg, _tracker())
    small = fd[:4, :, :96, :128].contiguous()
    a = [_snap(direct.process_device(fd[f])) for f in range(8)] + [_snap(direct.process_device(small[f])) for f in range(4)]
    b = [_snap(replayed.process_device(fd[f])) for f in range(8)]
    first = replayed.replays
    assert first > 0 and direct.replays == 0
    b += [_snap(replayed.process_device(small[f])) for f in range(4)]
    assert replayed.key[1:3] == (96, 128) and replayed.replays > first
    for i, (x, y) in enumerate(zip(a, b)):
        _bit_equal(y, x, i)
    assert sum(int(x['counts'].sum()) for x in a) > 0


def test_process_returns_the_demos_four_lists(stages):
    from torchdet3d.utils import FramePipeline, TrackedObj
    det, reg, frames, fd = stages
    pipe, lone = FramePipeline(det, reg, _tracker(1)), _tracker(1)
    for f in range(5):                                                # (crosses warm-up, recording and replay)
        detections, outputs, tracked, decoded = pipe.process(frames[f, 0])
        want = _hand(det, reg, lone, fd[f, :1])
        n, nt = int(want['counts'][0]), int(want['count'][0])
        assert detections == [(*want['rects'][0, i].tolist(), float(want['scores'][0, i]), int(want['det_labels'][0, i])) for i in range(n)]
        assert [o[1] for o in outputs] == want['labels'][0, :n].tolist()
        assert all(o[0].shape == (1, 9, 2) and np.array_equal(o[0].reshape(18), want['kp'][0, i]) for i, o in enumerate(outputs))
        assert tracked == [TrackedObj(tuple(want['boxes'][0, i].tolist()), tuple(want['track_kp'][0, i].tolist()), f"ID {want['ids'][0, i]}")
                           for i in range(nt)]
        assert len(decoded) == nt and all(np.array_equal(k.reshape(18), want['kp_frame'][0, i]) for i, k in enumerate(decoded))
    assert pipe.replays > 0


def test_frames_without_detections_age_and_clear_the_tracks(stages):
    """conf = 1.1: nothing passes, the tracker sees empty frames and ages / clears its tracks as it does on its own."""
    from torchdet3d.utils import FramePipeline
    det, reg, _, fd = stages
    pipe, lone = FramePipeline(det, reg, _tracker()), _tracker()
    conf = det.confidence
    try:
        for f in range(8):
            det.confidence = conf if f < 3 else 1.1
            got = _snap(pipe.process_device(fd[f]))
            if f < 3:
                assert got['counts'].sum() > 0
                rects, kp, counts = (torch.from_numpy(got[k]).cuda() for k in ('rects', 'kp', 'counts'))
            else:
                assert got['counts'].tolist() == [0] * S and got['overflow'].tolist() == [0] * S
                assert not got['rects'].any() and not got['scores'].any()
                counts = torch.zeros(S, dtype=torch.int32, device='cuda')
            lone.process_batch_device(rects, kp, counts)
            want = {k: v.cpu().numpy() for k, v in lone.tracked_device().items()}
            assert np.array_equal(got['count'], want['count']) and np.array_equal(got['scalars'], want['scalars']), f
            for s in range(S):
                n = want['count'][s]
                assert np.array_equal(got['boxes'][s, :n], want['boxes'][s, :n]) and np.array_equal(got['ids'][s, :n], want['ids'][s, :n])
        assert got['count'].tolist() == [0] * S
        assert (got['scalars'][:, 0] == 0).all(), 'every track has left through track_clear_thresh'
    finally:
        det.confidence = conf
