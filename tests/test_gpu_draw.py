"""GPU: the draw stage (csrc/draw.hip: t3d_draw_overlays_u8; torchdet3d/utils/draw.py) is bit-equal to the numpy restatement of
its raster rules (tests/draw_ref.py) on random-noise frames -- every byte of every frame, so a pixel no primitive covers keeps
its bytes -- through the byte-store and the dword-store paths, ragged tiles, a misaligned base, every optional input absent in
turn, keypoints that are no pixels, the full primitive mask, `draw_kp`, and as the last launch of `FramePipeline`, launch by
launch and replayed from the recorded plan.  tests/test_draw_host.py asserts that the scenes contain what they claim."""
import ctypes

import numpy as np
import pytest
import torch

import draw_ref as R
from draw_scenes import cube, many, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def glyphs():
    from torchdet3d import _native as N
    n = N.lib().t3d_draw_glyphs(None, 0)
    buf = (ctypes.c_ubyte * n)()
    assert N.lib().t3d_draw_glyphs(buf, n) == n
    return bytes(buf)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _check(sc, style, glyphs, use=('boxes', 'ids', 'labels', 'count'), label_count=None, misalign=False):
    """Draw the scene on the device and with the rules; every byte equal.  Returns the owner map."""
    from torchdet3d.utils import draw_overlays
    opt = {k: (sc[k] if k in use else None) for k in ('boxes', 'ids', 'labels', 'count')}
    S, H, W, _ = sc['frames'].shape
    if misalign:
        flat = torch.zeros(sc['frames'].size + 8, dtype=torch.uint8, device='cuda')
        base = 1 + (-flat.data_ptr()) % 4                              # an address that is 1 modulo 4
        frames = flat[base:base + sc['frames'].size].view(S, H, W, 3)
        frames.copy_(_dev(sc['frames']))
        assert frames.data_ptr() % 4 == 1
    else:
        frames = _dev(sc['frames'])
    out = draw_overlays(frames, _dev(sc['kp']), boxes=_dev(opt['boxes']), ids=_dev(opt['ids']), labels=_dev(opt['labels']),
                        count=_dev(opt['count']), label_count=_dev(label_count), style=style)
    assert out is frames
    want, own = R.draw_ref(sc['frames'], sc['kp'], glyphs, style.pack(), boxes=opt['boxes'], ids=opt['ids'], labels=opt['labels'],
                           count=opt['count'], label_count=label_count)
    got = frames.cpu().numpy()
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, f'{len(bad)} pixels differ, the first at (s, y, x) = {bad[0].tolist()}: owner {own[tuple(bad[0])]}'
    if misalign:
        assert not flat[:base].any() and not flat[base + sc['frames'].size:].any(), 'bytes outside the frames were written'
    return own


def _style(**kw):
    from torchdet3d.utils import DrawStyle
    return DrawStyle(**{**dict(font_scale=1, draw_ids=True), **kw})


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 37, 70), (2, 32, 64)], ids=['bytes-ragged', 'dwords'])
def test_scene_is_bit_equal_to_the_rules(shape, glyphs):
    own = _check(scene(*shape), _style(), glyphs)
    assert (own >= 0).any() and (own < 0).any()


def test_misaligned_frames_take_the_byte_path(glyphs):
    _check(scene(2, 32, 64), _style(), glyphs, misalign=True)


@pytest.mark.parametrize('th', [1, 2, 3, 5])
def test_thickness(th, glyphs):
    _check(scene(2, 32, 64), _style(rect_th=th, edge_th=th), glyphs)
    _check(scene(3, 37, 70), _style(rect_th=th, edge_th=6 - th), glyphs)


@pytest.mark.parametrize('radius', [0, 1, 4])
def test_disc_radius(radius, glyphs):
    _check(scene(3, 37, 70), _style(kp_radius=radius), glyphs)


@pytest.mark.parametrize('scale', [1, 2, 3])
def test_font_scale_with_and_without_ids(scale, glyphs):
    _check(scene(3, 37, 70), _style(font_scale=scale), glyphs)
    _check(scene(2, 32, 64), _style(font_scale=scale, draw_ids=False, bgr=True), glyphs)


@pytest.mark.parametrize('absent', ['boxes', 'ids', 'labels', 'count'])
def test_each_optional_input_absent(absent, glyphs):
    use = tuple(k for k in ('boxes', 'ids', 'labels', 'count') if k != absent)
    for shape in ((3, 37, 70), (2, 32, 64)):
        own = _check(scene(*shape), _style(), glyphs, use=use)
        if absent == 'count':
            assert all((own[s] >= 0).any() for s in range(shape[0])), 'a null count draws T objects on every camera'
        if absent == 'boxes':
            assert not (own % R.SLOTS == R.K_RECT)[own >= 0].any() and (own[-1, 0, 0] % R.SLOTS) >= R.K_PLATE


def test_label_count_cuts_the_labels(glyphs):
    sc = scene(3, 37, 70)
    for lc in ([5, 5, 2], [0, 0, 0], [9, -3, 99]):                     # (clamped to [0, stride])
        _check(sc, _style(draw_ids=False), glyphs, label_count=np.array(lc, np.int32))
    wide = dict(sc, labels=np.ascontiguousarray(np.tile(sc['labels'], (1, 2))))      # label_stride = 10 > T
    _check(wide, _style(), glyphs, label_count=np.array([1, 1, 4], np.int32))
    _check(wide, _style(), glyphs)


def test_keypoints_that_are_no_pixels(glyphs):
    """NaN, +-inf, +-9000 (past the limit), +-8191 and far off-frame but valid: skipped, or drawn as far as the frame goes."""
    rng = np.random.default_rng(4)
    S, H, W, T = 2, 37, 70, 6
    kp = np.stack([cube(14 + 9 * t, 10 + 3 * t, 7, 5) for _ in range(S) for t in range(T)]).reshape(S, T, 18)
    kp[:, 0, 2], kp[:, 0, 5] = np.nan, np.nan
    kp[:, 1, 4], kp[:, 1, 7] = np.inf, -np.inf
    kp[:, 2, 6], kp[:, 2, 9], kp[:, 2, 10] = 9000.0, -9000.0, 8191.5
    kp[:, 3, 2:4], kp[:, 3, 16:18] = (8191.0, -8191.0), (-8191.0, 8191.0)
    kp[:, 4, 8:10], kp[:, 4, 12:14] = (-4000.0, 2500.25), (3999.5, -2500.5)
    kp[:, 5] = np.nan
    sc = dict(frames=rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8), kp=kp, boxes=None, ids=None, labels=None, count=None)
    own = _check(sc, _style(edge_th=3), glyphs, use=())
    objs = set((own[own >= 0] // R.SLOTS).tolist())
    assert objs == {0, 1, 2, 3, 4}, 'an object of NaNs draws nothing'
    sc['boxes'] = np.tile(np.array([[-9000, -9000, 20, 20], [30, 9000, 9000, 10], [60, 5, 40, 30], [8191, 8191, -8192, -8192],
                                    [2 ** 31 - 1, 3, -2 ** 31, 30], [10, 10, 10, 10]], np.int32), (S, 1, 1))
    _check(sc, _style(rect_th=5), glyphs, use=('boxes',))


def test_the_full_primitive_mask(glyphs):
    sc = many()
    own = _check(sc, _style(rect_th=1, edge_th=1, kp_radius=1, draw_ids=False), glyphs)
    assert len(np.unique(own[own >= 0] // R.SLOTS)) > 300 and own.max() // R.SLOTS >= 1000 and (own < 0).any()


def test_no_cameras_and_bad_arguments():
    from torchdet3d import _native as N
    from torchdet3d.utils import DrawStyle
    lib, st = N.lib(), DrawStyle().pack()
    fr = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device='cuda')
    kp = torch.zeros(2, 4, 18, dtype=torch.float64, device='cuda')
    lab = torch.zeros(2, 2, dtype=torch.int32, device='cuda')
    f, k, la = fr.data_ptr(), kp.data_ptr(), lab.data_ptr()

    def call(frames=f, S=2, H=8, W=8, kpp=k, labels=None, lc=None, stride=0, T=4, style=st):
        return lib.t3d_draw_overlays_u8(frames, S, H, W, None, None, kpp, None, labels, lc, stride, T, style, N.stream())
    before = N.launch_count()
    assert call(S=0) == 0 and N.launch_count() == before, 'S = 0 is OK without a launch'
    for kw in (dict(frames=None), dict(kpp=None), dict(style=None), dict(S=-1), dict(S=65536), dict(H=0), dict(W=0), dict(H=8193),
               dict(W=8193), dict(T=0), dict(T=1025), dict(labels=la, stride=0), dict(labels=la, stride=2)):
        assert call(**kw) == -1, kw
    for field, bad in (('rect_th', 0), ('rect_th', 17), ('edge_th', 0), ('edge_th', 17), ('kp_radius', -1), ('kp_radius', 33),
                       ('font_scale', 0), ('font_scale', 9)):
        s2 = DrawStyle().pack()
        setattr(s2, field, bad)
        assert call(style=s2) == -1, (field, bad)
    assert N.launch_count() == before
    assert call(labels=la, lc=torch.zeros(2, dtype=torch.int32, device='cuda').data_ptr(), stride=2) == 0
    assert call() == 0 and N.launch_count() == before + 2
    torch.cuda.synchronize()
    from torchdet3d.utils import draw_overlays
    with pytest.raises(ValueError):
        draw_overlays(fr[:, :, ::2], kp)
    with pytest.raises(ValueError):
        draw_overlays(fr, kp.float())
    with pytest.raises(ValueError):
        draw_overlays(fr, kp, ids=torch.zeros(2, 3, dtype=torch.int32, device='cuda'))


# ---- draw_kp ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chw', [False, True], ids=['hwc', 'chw'])
@pytest.mark.parametrize('normalized', [True, False])
def test_draw_kp(chw, normalized, glyphs, tmp_path):
    from PIL import Image
    from torchdet3d.utils import DrawStyle, draw_kp
    rng = np.random.default_rng(9)
    H, W = 45, 61
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pix = cube(30, 22, 10, 7).reshape(9, 2)
    kp = pix / np.array([W, H]) if normalized else pix
    src = np.ascontiguousarray(img.transpose(2, 0, 1)) if chw else img
    name = str(tmp_path / 'kp.png')
    out = draw_kp(torch.from_numpy(src) if chw else src, kp, name, normalized=normalized, RGB=normalized, label='chair' if chw else 5)
    frame_kp = (kp * np.asarray([W, H], np.float64) if normalized else kp).reshape(1, 1, 18)
    want, own = R.draw_ref(img[None], frame_kp, glyphs, DrawStyle(bgr=not normalized).pack(), labels=np.array([[5]], np.int32))
    assert out.shape == (H, W, 3) and out.dtype == np.uint8 and np.array_equal(out, want[0])
    k = own[0] % R.SLOTS                                              # (T = 1: the slot is the layer; the plate hides edge 0)
    assert (own[0, :18, :62] >= R.K_PLATE).any() and ((own[0] >= 0) & (k >= R.K_EDGE0) & (k < R.K_DISC0)).any()
    assert ((own[0] >= 0) & (k >= R.K_DISC0) & (k < R.K_PLATE)).any()
    assert np.array_equal(src, np.ascontiguousarray(img.transpose(2, 0, 1)) if chw else img), 'the input is left alone'
    saved = np.asarray(Image.open(name).convert('RGB'))
    assert np.array_equal(saved, out if normalized else out[:, :, ::-1]), 'the file is RGB whatever the input order'


# ---- the last launch of the frame pipeline -----------------------------------------------------------------------------------------
S, D, H, W = 2, 8, 120, 160
TRACK = dict(time_window=2, continue_time_thresh=2, track_clear_thresh=3)


@pytest.fixture(scope='module')
def stages():
    """The small stages of tests/test_gpu_frame_pipeline.py: seeded SSD300 (bf16) + mobilenetv2 regressor on 96 x 96 crops,
    8 frames of S = 2 cameras, the confidence midway between the 5th and 6th best score of camera 0's first frame."""
    from oracle.weights import make_state_dict
    from test_gpu_two_stage import _ssd_pair
    from test_host_logic import _cfg
    from torchdet3d.builders import build_model
    from torchdet3d.utils import Detector, Regressor
    m, _, _, _ = _ssd_pair(torch.bfloat16)
    cfg = _cfg('mobilenetv2')
    cfg.model.storage_dtype = 'bf16'
    model = build_model(cfg, export_mode=True).to('cuda')
    model.load_state_dict(make_state_dict('mobilenetv2', 9))
    reg = Regressor(model, (96, 96))
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (8, S, H, W, 3), dtype=np.uint8)
    det = Detector(m, conf=0.0)
    img, _ = det._enqueue(frames[0, 0])
    sc = np.sort(m.detect(img)[0][:, 4])[::-1]
    assert len(sc) >= 6 and sc[4] > sc[5]
    det.confidence = float((np.float64(sc[4]) + np.float64(sc[5])) / 2)
    return det, reg, frames


def _tracker():
    from torchdet3d.utils import IOUTracker
    return IOUTracker(**TRACK, device='cuda', streams=S, max_detections=D, max_tracks=16)


def _snap(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in res.items()}


def test_frame_pipeline_draws_what_it_returns(stages, glyphs, monkeypatch):
    from torchdet3d.utils import DrawStyle, FramePipeline
    det, reg, frames = stages
    style = DrawStyle(draw_ids=True)
    monkeypatch.setenv('T3D_STEP_PLAN', '0')
    plain, direct = FramePipeline(det, reg, _tracker()), FramePipeline(det, reg, _tracker(), draw=style)
    monkeypatch.delenv('T3D_STEP_PLAN')
    replayed = FramePipeline(det, reg, _tracker(), draw=style)
    drawn, tracked = 0, 0
    for f in range(8):
        fa, fb, fc = (torch.from_numpy(frames[f]).cuda() for _ in range(3))        # three copies at three addresses
        a, b, c = _snap(plain.process_device(fa)), _snap(direct.process_device(fb)), _snap(replayed.process_device(fc))
        for k in a:
            assert a[k].dtype == b[k].dtype == c[k].dtype and a[k].shape == b[k].shape == c[k].shape, k
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), ('drawing changed a result', f, k)
            assert np.array_equal(a[k].view(np.uint8), c[k].view(np.uint8)), ('the replayed chain differs', f, k)
        assert np.array_equal(fa.cpu().numpy(), frames[f]), 'draw=None leaves the frames alone'
        want, own = R.draw_ref(frames[f], b['kp_frame'], glyphs, style.pack(), boxes=b['boxes'], ids=b['ids'], labels=b['labels'],
                               count=b['count'], label_count=b['counts'])
        got = fb.cpu().numpy()
        bad = np.argwhere((got != want).any(-1))
        assert bad.size == 0, f'frame {f}: {len(bad)} pixels differ, the first at {bad[0].tolist()}'
        assert np.array_equal(fc.cpu().numpy(), got), ('replayed frames differ from launch-by-launch ones', f)
        drawn += int((own >= 0).sum())
        tracked += int(((own >= 0) & (own % R.SLOTS >= R.K_EDGE0) & (own % R.SLOTS < R.K_PLATE)).sum())
    assert plain.replays == 0 and direct.replays == 0 and replayed.replays > 0
    assert drawn > 0 and tracked > 0, 'rectangles, and the boxes of tracks old enough to carry an id, were drawn'
    with pytest.raises(ValueError):
        FramePipeline(det, reg, _tracker(), draw='green')
