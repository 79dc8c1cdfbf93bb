"""GPU: `t3d_jpeg_encode_u8` (csrc/jpeg_encode.hip) byte for byte against the numpy restatement tests/jpeg_encode_ref.py (which
tests/test_jpeg_encode_host.py pins to Pillow on libjpeg-turbo) -- sizes with dummy blocks on either edge, both samplings, four
qualities, the extreme contents, every segment length -- and against Pillow itself for a 1080 x 1920 frame; the overflow rows
with guard bytes around the slots and the workspace; determinism and streams; the refusals; `JpegEncoder`; and the round trip
encoder -> MjpegWriter -> MjpegReader -> JpegIndex rows -> t3d_jpeg_decode_u8."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image, features

import jpeg_encode_cases as C
import jpeg_encode_ref as R

pytestmark = pytest.mark.gpu
GUARD, FILL, HEADER = 256, 0xEE, 623
_want = {}


def want(frame_key, frame, q, s):
    """The restatement's file, computed once per (frame, quality, sampling)."""
    k = (frame_key, q, s)
    if k not in _want:
        _want[k] = R.encode(frame, q, s)
    return _want[k]


def run(frames, q, s, seg_mcus=None, cap=None):
    """One t3d_jpeg_encode_u8 call on the current stream: frames numpy [B, h, w, 3].  FILL in every slot, GUARD bytes of it behind
    `out` and around the workspace.  -> (result rows, out numpy [B, cap], guards untouched)."""
    from torchdet3d import _native as N
    from torchdet3d.utils.jpeg_encode import DEFAULT_ENC_SEG_MCUS, ENC_RESULT_DTYPE, encode_tables
    B, h, w = frames.shape[:3]
    seg_mcus = DEFAULT_ENC_SEG_MCUS if seg_mcus is None else seg_mcus
    cap = 3 * h * w * 3 + 1024 if cap is None else cap              # (noise at quality 100 is larger than the raw frame)
    rc, tables = encode_tables(h, w, q, s)
    assert rc == 0
    nbytes = ctypes.c_longlong(0)
    assert N.lib().t3d_jpeg_encode_work_bytes(B, h, w, s, seg_mcus, cap, ctypes.byref(nbytes)) == 0
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    tdev = torch.from_numpy(tables.view(np.uint8).copy()).cuda()
    out = torch.full((B * cap + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    arena = torch.full((nbytes.value + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    work = arena[GUARD:GUARD + nbytes.value]                                   # (16-byte aligned, as the call demands)
    results = torch.full((B * 16,), 0x77, dtype=torch.uint8, device='cuda')
    N.call('t3d_jpeg_encode_u8', N.ptr(dev), B, tables.ctypes.data, N.ptr(tdev), seg_mcus, N.ptr(out), cap, N.ptr(results),
           work.data_ptr(), nbytes.value, N.stream())
    torch.cuda.synchronize()
    o, a = out.cpu().numpy(), arena.cpu().numpy()
    clean = bool(np.all(o[B * cap:] == FILL) and np.all(a[:GUARD] == FILL) and np.all(a[GUARD + nbytes.value:] == FILL))
    return results.cpu().numpy().view(ENC_RESULT_DTYPE), o[:B * cap].reshape(B, cap), clean


def files_of(res, out):
    """The files of a call whose frames all fit; the rest of every slot still holds FILL."""
    assert not res['overflow'].any() and not res['reserved'].any(), res
    for i in range(len(res)):
        assert np.all(out[i, int(res['bytes'][i]):] == FILL), f'slot {i} was written behind its file'
    return [out[i, :int(res['bytes'][i])].tobytes() for i in range(len(res))]


def trio(h, w):
    return np.stack([C.noise(h, w), C.smooth(h, w), C.checker(h, w)])


# ---- bytes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(8, 8), (16, 16), (33, 17), (40, 56), (270, 480)])
def test_files_equal_the_restatements(h, w):
    frames = trio(h, w)
    for s in C.SAMPLINGS:
        for q in (1, 50, 90, 100):
            res, out, clean = run(frames, q, s)
            assert clean, 'a byte behind out or outside the workspace was written'
            for i, got in enumerate(files_of(res, out)):
                assert got == want((h, w, i), frames[i], q, s), (h, w, s, q, i)


@pytest.mark.parametrize('s', C.SAMPLINGS)
def test_extreme_contents(s):
    """ZRL runs, the longest codes, dense FF stuffing: six contents at 24 x 40 in one call, quality 100."""
    names, frames = zip(*C.extremes())
    res, out, clean = run(np.stack(frames), 100, s)
    assert clean
    got = files_of(res, out)
    for i, name in enumerate(names):
        assert got[i] == want(('extreme', i), frames[i], 100, s), name
    assert any(g.count(b'\xff\x00') > 20 for g in got), 'no case with dense stuffing'


@pytest.mark.parametrize('h,w', [(33, 17), (270, 480)])
def test_every_segment_length_gives_the_same_bytes(h, w):
    frames = trio(h, w)
    nmcu = -(-h // 16) * -(-w // 16)
    for seg in (1, 2, 3, 7, nmcu + 5):
        res, out, clean = run(frames, 90, 2, seg_mcus=seg)
        assert clean
        for i, got in enumerate(files_of(res, out)):
            assert got == want((h, w, i), frames[i], 90, 2), (seg, i)
    res, out, clean = run(frames, 100, 1, seg_mcus=7)
    assert clean and files_of(res, out) == [want((h, w, i), frames[i], 100, 1) for i in range(3)]


def test_large_frames_are_pillows_files_and_decode_on_the_device_to_pillows_pixels():
    assert features.check_feature('libjpeg_turbo')
    from torchdet3d.dataloaders.jpeg import decode_jpeg_batch, index_jpeg
    h, w = 1080, 1920
    frames = np.stack([C.drawn(h, w, 0), C.drawn(h, w, 1)])
    res, out, clean = run(frames, 90, 2, cap=1 << 20)
    assert clean
    got = files_of(res, out)
    for i in range(2):
        assert got[i] == C.pillow(frames[i], 90, 2), i
    rows = []
    for f in got:
        rc, info, segs = index_jpeg(f)
        assert rc == 0 and int(info['reason']) == 0
        rows.append((info, segs))
    packed, desc = decode_jpeg_batch(got, rows)
    torch.cuda.synchronize()
    assert not decode_jpeg_batch.last_status.cpu().numpy().any()
    packed = packed.cpu().numpy()
    for i, f in enumerate(got):
        off = int(desc[i, 0])
        assert np.array_equal(packed[off:off + h * w * 3].reshape(h, w, 3), np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))), i


# ---- overflow ------------------------------------------------------------------------------------------------------------------------
def test_a_frame_that_does_not_fit_is_flagged_and_the_others_are_exact():
    from torchdet3d.utils import JpegEncoder
    h, w, q, s = 40, 56, 100, 1
    frames = sorted((C.noise(h, w, k) for k in range(3)), key=lambda f: len(want(('of', f.tobytes()), f, q, s)))
    frames = np.stack([frames[0], frames[2], frames[1]])                  # the largest file in the middle
    files = [want(('of', f.tobytes()), f, q, s) for f in frames]
    cap = max(len(files[0]), len(files[2]))
    assert cap < len(files[1])
    res, out, clean = run(frames, q, s, cap=cap)
    assert clean
    assert list(res['overflow']) == [0, 1, 0] and not res['reserved'].any()
    assert int(res['bytes'][1]) == HEADER + R.unstuffed_scan_bytes(frames[1], q, s) + 2 <= len(files[1]) <= 2 * int(res['bytes'][1])
    for i in (0, 2):
        assert out[i, :int(res['bytes'][i])].tobytes() == files[i], i
        assert np.all(out[i, int(res['bytes'][i]):] == FILL)
    assert np.all(out[1] == FILL), 'the frame that does not fit wrote into its slot'
    # (there the scan fitted its share of the work buffer and the stuffed file did not fit the slot.)  A slot far smaller than
    # the middle frame's scan: the emit lanes of that frame leave, the others are exact
    mixed = np.stack([C.smooth(h, w), frames[1], C.smooth(h, w)[::-1].copy()])
    mfiles = [want(('of', f.tobytes()), f, q, s) for f in mixed]
    cap2 = max(len(mfiles[0]), len(mfiles[2]))
    assert -(-cap2 // 64) * 64 < R.unstuffed_scan_bytes(mixed[1], q, s)
    res2, out2, clean2 = run(mixed, q, s, cap=cap2)
    assert clean2 and list(res2['overflow']) == [0, 1, 0] and int(res2['bytes'][1]) == int(res['bytes'][1])
    assert np.all(out2[1] == FILL)
    for i in (0, 2):
        assert out2[i, :int(res2['bytes'][i])].tobytes() == mfiles[i] and np.all(out2[i, int(res2['bytes'][i]):] == FILL), i
    enc = JpegEncoder(h, w, quality=q, sampling='444', max_frames=3, cap_bytes=cap)
    assert enc.encode(torch.from_numpy(frames).cuda()) == files
    assert JpegEncoder(h, w, quality=q, sampling='444', max_frames=3, cap_bytes=cap2).encode(torch.from_numpy(mixed).cuda()) == mfiles


# ---- determinism, streams, the wrapper -----------------------------------------------------------------------------------------------
def test_two_calls_and_another_stream_give_the_same_bytes():
    from torchdet3d.utils import JpegEncoder
    h, w = 270, 480
    frames = trio(h, w)
    a = run(frames, 90, 2)
    b = run(frames, 90, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] and b[2]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = run(frames, 90, 2)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and c[2]
    enc = JpegEncoder(h, w, max_frames=4)
    assert (enc.quality, enc.sampling, enc.cap_bytes) == (90, 2, h * w * 3)
    dev = torch.from_numpy(frames).cuda()
    files = [want((h, w, i), frames[i], 90, 2) for i in range(3)]
    assert enc.encode(dev) == files and enc.encode(dev[1]) == files[1:2]
    out, results = enc.encode_device(dev[:2])
    assert out.shape == (2, h * w * 3) and results.shape == (2, 16) and out.is_cuda and results.is_cuda
    side.wait_stream(torch.cuda.current_stream())        # (the encoder's buffers are shared by its calls: the caller orders streams)
    with torch.cuda.stream(side):
        assert enc.encode(dev) == files
    side.synchronize()


def test_refusals():
    from torchdet3d import _native as N
    from torchdet3d.utils import JpegEncoder
    from torchdet3d.utils.jpeg_encode import encode_tables
    lib = N.lib()
    h, w = 33, 17
    _, t = encode_tables(h, w, 90, 2)
    dev = torch.from_numpy(trio(h, w)).cuda()
    tdev = torch.from_numpy(t.view(np.uint8).copy()).cuda()
    cap = 4096
    nb = ctypes.c_longlong(0)
    assert lib.t3d_jpeg_encode_work_bytes(3, h, w, 2, 2, cap, ctypes.byref(nb)) == 0
    out = torch.full((3 * cap,), FILL, dtype=torch.uint8, device='cuda')
    results = torch.full((3 * 16,), 0x77, dtype=torch.uint8, device='cuda')
    work = torch.empty(nb.value + 16, dtype=torch.uint8, device='cuda')
    good = [N.ptr(dev), 3, t.ctypes.data, N.ptr(tdev), 2, N.ptr(out), cap, N.ptr(results), N.ptr(work), nb.value, N.stream()]
    launches = N.launch_count()
    for i, v in ((0, None), (1, -1), (1, 65536), (2, None), (3, None), (4, 0), (5, None), (5, N.ptr(out) + 4), (6, HEADER + 1), (7, None),
                 (8, None), (8, N.ptr(work) + 8), (9, nb.value - 1)):
        args = list(good)
        args[i] = v
        assert lib.t3d_jpeg_encode_u8(*args) == N.ERR_ARG, (i, v)
    args = list(good)
    args[1] = 0
    assert lib.t3d_jpeg_encode_u8(*args) == 0
    assert N.launch_count() == launches, 'a refused call or B == 0 launched a kernel'
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((results == 0x77).all())
    assert lib.t3d_jpeg_encode_u8(*good) == 0 and N.launch_count() == launches + 7
    torch.cuda.synchronize()
    for bad in (dict(h=0), dict(w=70000), dict(quality=0), dict(quality=101), dict(sampling='422'), dict(max_frames=0), dict(seg_mcus=0),
                dict(cap_bytes=HEADER + 1)):
        with pytest.raises(ValueError):
            JpegEncoder(**{**dict(h=h, w=w), **bad})
    enc = JpegEncoder(h, w, max_frames=2)
    for frames in (dev, dev[:2].cpu(), dev[:2].float(), dev[:2, :, :16], dev[:2, :32], dev[:2].permute(0, 2, 1, 3), dev[:2, ..., :2],
                   dev[0, 0], np.zeros((h, w, 3), np.uint8)):
        with pytest.raises(ValueError):
            enc.encode_device(frames)


# ---- the container -------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_container(tmp_path):
    assert features.check_feature('libjpeg_turbo')
    from torchdet3d.dataloaders.jpeg import decode_jpeg_batch, index_jpeg
    from torchdet3d.utils import JpegEncoder, MjpegReader, MjpegWriter
    h, w = 270, 480
    frames = np.stack([C.drawn(h, w, k) for k in range(4)])
    enc = JpegEncoder(h, w, quality=90, sampling='420', max_frames=4)
    files = enc.encode(torch.from_numpy(frames).cuda())
    path = str(tmp_path / 'out.avi')
    with MjpegWriter(path, 30, (w, h)) as wr:
        for f in files:
            wr.write(f)
    with MjpegReader(path) as rd:
        assert (rd.fps, rd.size, len(rd)) == (30.0, (w, h), 4)
        back = list(rd)
    assert back == files
    rows = []
    for f in back:
        rc, info, segs = index_jpeg(f)
        assert rc == 0
        rows.append((info, segs))
    packed, desc = decode_jpeg_batch(back, rows)
    torch.cuda.synchronize()
    packed = packed.cpu().numpy()
    for i, f in enumerate(back):
        off = int(desc[i, 0])
        assert np.array_equal(packed[off:off + h * w * 3].reshape(h, w, 3), np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))), i
