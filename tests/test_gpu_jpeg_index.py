"""GPU: the MCU index built on the device (t3d_jpeg_index_device; csrc/jpeg_scan.h, csrc/jpeg_scan.hip) against the host indexer
t3d_jpeg_index -- rows, records and status byte for byte, guard bytes around every buffer the call writes --, the decode chained
behind it against Pillow, refusals inside a mixed batch, the saved index built on the device, and Motion-JPEG frames handed to
the frame pipeline."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as C

pytestmark = pytest.mark.gpu
GUARD, POISON = 64, 0xA5
ONE_PER_IMAGE = 1 << 30
ONE_LANE = 1 << 20


def _J():
    from torchdet3d.dataloaders import jpeg as J
    return J


_host = {}


def _host_rows(seg_mcus):
    """The host indexer's (infos, segs) of the 270-file matrix, made once per seg_mcus."""
    if seg_mcus not in _host:
        J = _J()
        rows = [J.index_jpeg(d, seg_mcus) for _, d in C.matrix()]
        assert all(r[0] == 0 for r in rows)
        _host[seg_mcus] = (np.array([r[1] for r in rows], J.INFO_DTYPE), np.concatenate([r[2] for r in rows]))
    return _host[seg_mcus]


def _guarded(nbytes, dev):
    t = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
    return t, t.data_ptr() + GUARD


def _intact(t, nbytes):
    h = t.cpu().numpy()
    return bool((h[:GUARD] == POISON).all() and (h[GUARD + nbytes:] == POISON).all())


def _index_guarded(files, seg_mcus, sub):
    """One t3d_jpeg_index_device call with every written buffer between guard bytes -> (infos, segs, status) as numpy."""
    from torchdet3d import _native as N
    J = _J()
    dev = torch.device('cuda', torch.cuda.current_device())
    arrs = [np.frombuffer(f, np.uint8) for f in files]
    B = len(arrs)
    heads = np.zeros(B, J.INFO_DTYPE)
    for i, a in enumerate(arrs):
        rc, heads[i] = J.read_jpeg_header(a, seg_mcus)
        assert rc == 0
    sizes = np.array([a.size for a in arrs], np.int64)
    nseg, nsub = heads['nseg'].astype(np.int64), -(-heads['scan_bytes'].astype(np.int64) // sub)
    items = np.zeros(B, J.ITEM_DTYPE)
    items['file_offset'], items['file_bytes'] = np.cumsum(sizes) - sizes, sizes
    items['seg_offset'], items['block_offset'] = np.cumsum(nseg) - nseg, np.cumsum(nsub) - nsub
    data = torch.from_numpy(np.concatenate(arrs)).to(dev)
    d_items = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    total = int(nseg.sum())
    nbytes = ctypes.c_longlong(0)
    assert N.lib().t3d_jpeg_index_work_bytes(int(heads['scan_bytes'].sum()), B, sub, ctypes.byref(nbytes)) == 0
    sizes_b = dict(infos=B * 864, segs=total * 16, status=B * 4, work=nbytes.value)
    buf = {k: _guarded(v, dev) for k, v in sizes_b.items()}
    buf['infos'][0][GUARD:GUARD + B * 864] = torch.from_numpy(heads.view(np.uint8).copy()).to(dev)
    N.call('t3d_jpeg_index_device', data.data_ptr(), data.numel(), buf['infos'][1], buf['segs'][1], total, d_items.data_ptr(), sub,
           buf['work'][1], nbytes.value, buf['status'][1], B, int(nsub.max()), N.stream())
    torch.cuda.synchronize()
    for k, v in sizes_b.items():
        assert _intact(buf[k][0], v), f'guard bytes around {k} were written'
    host = {k: buf[k][0].cpu().numpy()[GUARD:GUARD + v] for k, v in sizes_b.items()}
    return host['infos'].view(J.INFO_DTYPE), host['segs'].view(J.SEG_DTYPE), host['status'].view(np.int32)


@pytest.mark.parametrize('lanes', ['smallest', 'default', 'one'])
@pytest.mark.parametrize('seg_mcus', [1, 2, 3, ONE_PER_IMAGE])
def test_the_device_rows_are_the_host_indexers(seg_mcus, lanes):
    J = _J()
    sub = dict(smallest=J.SUB_BYTES_RANGE[0], default=J.DEFAULT_SUB_BYTES, one=ONE_LANE)[lanes]
    want_infos, want_segs = _host_rows(seg_mcus)
    infos, segs, status = _index_guarded([d for _, d in C.matrix()], seg_mcus, sub)
    assert not status.any()
    assert segs.tobytes() == want_segs.tobytes()
    assert infos.tobytes() == want_infos.tobytes()


def test_the_chained_decode_equals_pillow():
    J = _J()
    q = C.QUALITIES.index((90, False))
    subset = [C.matrix()[k] for k in range(q, 270, len(C.QUALITIES))]          # each size, each sampling, one quality
    assert len(subset) == 45
    packed, desc = J.decode_jpeg_frames([d for _, d in subset])
    a, b = (s.cpu().numpy() for s in J.decode_jpeg_frames.last_status)
    assert not a.any() and not b.any()
    out = packed.cpu().numpy()
    for (name, data), (off, h, w) in zip(subset, desc):
        assert np.array_equal(out[off:off + h * w * 3].reshape(h, w, 3), C.pillow(data)), name


def test_refused_scans_inside_a_batch_leave_their_neighbours_alone():
    J = _J()
    base, corpus = C.malformed()
    rc, info, _ = J.index_jpeg(base)
    assert rc == 0
    so, sb = int(info['scan_offset']), int(info['scan_bytes'])
    truncated, cut_eoi = corpus[so + sb // 2], corpus[len(base) - 1]
    mutated = next(m for m in corpus[len(base):] if J.read_jpeg_header(m)[0] == 0 and J.index_jpeg(m)[0] == -1
                   and m[:so] == base[:so] and m[so + sb:] == base[so + sb:])      # one byte of the scan replaced
    good = [C.matrix()[k][1] for k in (100, 130, 160, 190)]
    files = [good[0], truncated, good[1], mutated, good[2], cut_eoi, good[3]]
    bad = [1, 3, 5]
    for k in bad:
        assert J.read_jpeg_header(files[k])[0] == 0 and J.index_jpeg(files[k])[0] == -1
    d = J._index_device(files, J.DEFAULT_SEG_MCUS, J.DEFAULT_SUB_BYTES, None, decode=True)
    sizes = [(int(h['h']), int(h['w'])) for h in d['heads']]
    out, desc = J._packed(sizes, d['status'].device)
    out.fill_(POISON)
    dec = J.launch_decode(d['data'], d['infos'], d['segs'], d['items'], d['plan'], out).cpu().numpy()
    idx = d['status'].cpu().numpy()
    assert idx.tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert dec.tolist() == [0, 2, 0, 2, 0, 2, 0]
    infos = d['infos'].cpu().numpy().view(J.INFO_DTYPE)
    assert (infos['scan_bytes'][bad] == -1).all()
    host = out.cpu().numpy()
    for k, (off, h, w) in enumerate(desc):
        got = host[off:off + h * w * 3]
        if k in bad:
            assert (got == POISON).all(), k
        else:
            assert np.array_equal(got.reshape(h, w, 3), C.pillow(files[k])), k


def test_an_index_built_on_the_device_equals_the_host_build(tmp_path):
    J = _J()
    base, corpus = C.malformed()
    so = int(J.index_jpeg(base)[1]['scan_offset'])
    files = {f'{k:02d}.jpg': C.matrix()[20 * k + 3][1] for k in range(10)}
    files['p.jpg'] = C.encode(C.image(24, 40, 9), '420', 90, progressive=True)
    files['t.jpg'] = corpus[so + 60]                                         # cut inside its scan: the device's status 1
    for name, data in files.items():
        with open(tmp_path / name, 'wb') as f:
            f.write(data)
    names = sorted(files)
    host = J.JpegIndex.build(names, str(tmp_path), seg_mcus=2)
    dev = J.JpegIndex.build(names, str(tmp_path), seg_mcus=2, where='device')
    assert host.reason.tolist().count(0) == 10 and 1 in host.reason and -1 in host.reason
    for field in ('infos', 'segs', 'seg_start', 'size', 'mtime_ns', 'reason'):
        a, b = getattr(host, field), getattr(dev, field)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), field
    assert dev.files == host.files and dev.seg_mcus == host.seg_mcus


@pytest.mark.parametrize('h,w,n', [(48, 64, 5), (1080, 1920, 3)])
def test_motion_jpeg_frames_reach_the_pipeline_from_the_device(tmp_path, h, w, n):
    from torchdet3d.utils import MjpegReader, MjpegWriter
    chunks = [C.encode(C.image(h, w, 40 + k), '420', 90) for k in range(n)]
    path = str(tmp_path / 'v.avi')
    with MjpegWriter(path, 30, (w, h)) as wr:
        for c in chunks:
            wr.write(c)
    with MjpegReader(path) as rd:
        frames, (a, b) = rd.frames_device(0, n)
        tail, _ = rd.frames_device(n - 1, 1)
        with pytest.raises(ValueError):
            rd.frames_device(n - 1, 2)
    # what FramePipeline.process_device takes, as it stands: uint8 [S, H, W, 3], contiguous, on the device, its own storage's start
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (n, h, w, 3) and frames.is_contiguous()
    assert frames.data_ptr() == frames.untyped_storage().data_ptr()
    assert not a.cpu().numpy().any() and not b.cpu().numpy().any()
    got = frames.cpu().numpy()
    for k, c in enumerate(chunks):
        assert np.array_equal(got[k], np.asarray(Image.open(io.BytesIO(c)).convert('RGB'))), k
    assert np.array_equal(tail.cpu().numpy()[0], got[n - 1])


def test_one_call_is_four_kernels_whatever_the_batch():
    from torchdet3d import _native as N
    J = _J()
    files = [d for _, d in C.matrix()]
    for B in (1, 64):
        torch.cuda.synchronize()
        before = N.launch_count()
        J.index_jpeg_device(files[100:100 + B])
        assert N.launch_count() - before == 4, B
    torch.cuda.synchronize()
