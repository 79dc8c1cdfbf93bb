"""CPU: the host half of the device JPEG decode (csrc/jpeg_index.h, torchdet3d/dataloaders/jpeg.py).  The numpy restatement
tests/jpeg_ref.py against Pillow on libjpeg-turbo bit for bit; `t3d_jpeg_index` against Pillow's header, its segment tables
against the sequential decode, its reasons for the files it leaves to the host, its behaviour on truncated and mutated files;
`JpegIndex` on disk and against changed files; and that no DataLoader worker touches the native library.

T3D_JPEG_CORPUS=DIR makes the malformed-file test also write its corpus to DIR, for tools/jpeg_index_check.cpp."""
import io
import json
import os

import numpy as np
import pytest
from PIL import Image, features

import jpeg_cases as C
import jpeg_ref as R

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3


def _J():
    from torchdet3d.dataloaders import jpeg
    return jpeg


def test_the_restatement_equals_pillow_bit_for_bit():
    assert features.check_feature('libjpeg_turbo'), 'the pixels are pinned on libjpeg-turbo'
    for name, data in C.matrix():
        assert np.array_equal(R.decode(data), C.pillow(data)), name


def test_the_index_reports_what_pillow_reads():
    J = _J()
    for name, data in C.matrix():
        rc, info, segs = J.index_jpeg(data, 4)
        im = Image.open(io.BytesIO(data))
        assert rc == OK, name
        assert (int(info['w']), int(info['h'])) == im.size and int(info['ncomp']) == len(im.getbands()), name
        px = 16 if '_420_' in name else 8
        assert int(info['mcus_x']) == -(-im.size[0] // px) and int(info['mcus_y']) == -(-im.size[1] // px)
        nmcu = int(info['mcus_x']) * int(info['mcus_y'])
        assert int(info['nseg']) == len(segs) == -(-nmcu // 4) and int(info['reason']) == 0
        assert np.array_equal(segs['mcu'], 4 * np.arange(len(segs)))
        p = R.parse(data)
        assert int(info['scan_offset']) == p['scan'] and data[p['scan'] + int(info['scan_bytes']):][:2] == b'\xff\xd9'
        for c in range(p['ncomp']):
            assert np.array_equal(info['quant'][c], p['quant'][c])


@pytest.mark.parametrize('seg_mcus', [1, 3, 8, 1 << 20])
def test_decoding_from_the_index_equals_the_sequential_decode(seg_mcus):
    J = _J()
    picked = [(n, d) for n, d in C.matrix() if n.split('_')[0] in ('1x1', '49x2', '17x33', '37x53', '40x56') and '_q35_' in n]
    assert len(picked) == 15
    for name, data in picked:
        rc, info, segs = J.index_jpeg(data, seg_mcus)
        assert rc == OK and (seg_mcus < (1 << 20) or len(segs) == 1), name
        assert np.all(segs['byte'] < int(info['scan_bytes'])) and np.all(segs['bit'] < 8)
        assert np.array_equal(R.decode(data, segs, seg_mcus), R.decode(data)), name


def test_unsupported_files_say_why():
    J = _J()
    img = C.image(40, 56, 1)
    cmyk = io.BytesIO()
    Image.fromarray(np.concatenate([img, img[..., :1]], -1), 'CMYK').save(cmyk, format='JPEG', quality=90)
    files = {'progressive': C.encode(img, '420', 90, progressive=True), '4:2:2': C.encode(img, '422', 90),
             'restart markers': C.encode(img, '420', 90, restart_marker_rows=1), 'CMYK': cmyk.getvalue()}
    reasons = {}
    for what, data in files.items():
        rc, info, _ = J.index_jpeg(data)
        assert rc == ERR_UNSUPPORTED, what
        reasons[what] = int(info['reason'])
    assert reasons == {'progressive': 1, 'restart markers': 3, '4:2:2': 4, 'CMYK': 5}
    assert all(r in J.REASONS for r in reasons.values())


def test_truncated_and_mutated_files_never_crash_and_accepted_tables_stay_inside_the_scan():
    J = _J()
    base, corpus = C.malformed()
    out = os.environ.get('T3D_JPEG_CORPUS')
    if out:
        C.write_files(out, corpus)
    seen = set()
    for data in corpus:
        rc, info, segs = J.index_jpeg(data, 2)
        assert rc in (OK, ERR_ARG, ERR_UNSUPPORTED)
        seen.add(rc)
        if rc == OK:
            so, sb = int(info['scan_offset']), int(info['scan_bytes'])
            assert 0 < so and 0 < sb and so + sb <= len(data) and len(segs) == int(info['nseg']) >= 1
            assert np.all(segs['byte'] < sb) and np.all(segs['bit'] < 8)
    assert all(J.index_jpeg(d, 2)[0] == ERR_ARG for d in corpus[:len(base)]), 'a truncated file was accepted'
    assert seen >= {OK, ERR_ARG}


def _dataset(root, files):
    """files: {name: bytes} -> an Objectron-style folder with one box per image."""
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    images, anns = [], []
    for i, (name, data) in enumerate(files.items()):
        with open(os.path.join(root, 'images', name), 'wb') as f:
            f.write(data)
        w, h = Image.open(io.BytesIO(data)).size
        images.append(dict(id=i + 1, file_name='images/' + name, width=w, height=h))
        anns.append(dict(id=i, image_id=i + 1, category_id=1 + i % 9, iscrowd=0, bbox=[1.0, 2.0, w * .5, h * .5]))
    for name in ('objectron_train.json', 'objectron_test.json'):
        with open(os.path.join(root, 'annotations', name), 'w') as f:
            json.dump(dict(images=images, annotations=anns, categories=[]), f)


def _files():
    return {f'{i}.jpg': C.encode(C.image(h, w, i), s, 90) for i, (h, w, s) in
            enumerate([(40, 56, '420'), (33, 17, '444'), (24, 40, 'gray'), (37, 53, '420')])}


def test_the_index_round_trips_through_npy_and_npz_and_maps(tmp_path):
    J = _J()
    files = _files()
    files['p.jpg'] = C.encode(C.image(24, 40, 9), '420', 90, progressive=True)
    _dataset(str(tmp_path), files)
    names = ['images/' + n for n in files]
    idx = J.JpegIndex.build(names, str(tmp_path), seg_mcus=3, threads=4)
    assert list(idx.reason) == [0, 0, 0, 0, 1] and idx.seg_start[-1] == len(idx.segs) and idx.seg_start[4] == idx.seg_start[5]
    for path, mm in ((tmp_path / 'i.npy', 'r'), (tmp_path / 'i.npy', None), (tmp_path / 'i.npz', None)):
        idx.save(path)
        back = J.JpegIndex.load(path, mmap_mode=mm)
        assert isinstance(back.infos, np.memmap) == (mm == 'r')
        assert back.files == names and back.seg_mcus == 3
        for a, b in ((idx.infos, back.infos), (idx.segs, back.segs), (idx.seg_start, back.seg_start), (idx.size, back.size),
                     (idx.mtime_ns, back.mtime_ns), (idx.reason, back.reason)):
            assert a.dtype == b.dtype and np.array_equal(np.asarray(a), np.asarray(b))
        info, segs = back.rows(3)
        assert np.array_equal(R.decode(files['3.jpg'], segs, 3), C.pillow(files['3.jpg']))
        back.check(str(tmp_path))


def test_a_file_that_changed_since_it_was_indexed_raises_naming_it(tmp_path):
    from torchdet3d.dataloaders import ObjectronFrames
    files = _files()
    _dataset(str(tmp_path), files)
    ds = ObjectronFrames(str(tmp_path), 'train', decode='device')
    with pytest.raises(RuntimeError, match='build_index'):
        ds[0]
    ds.build_index(str(tmp_path / 'idx.npy'), threads=2)
    payload, boxes, labels, i = ds[1]
    assert payload.dtype == np.uint8 and payload.tobytes() == files['1.jpg'] and i == 1
    victim = os.path.join(str(tmp_path), 'images', '2.jpg')
    st = os.stat(victim)
    os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))                  # the mtime alone
    with pytest.raises(RuntimeError, match='2.jpg'):
        ObjectronFrames(str(tmp_path), 'train', decode='device').build_index(str(tmp_path / 'idx.npy'))
    os.utime(victim, ns=(st.st_atime_ns, st.st_mtime_ns))
    ObjectronFrames(str(tmp_path), 'train', decode='device').build_index(str(tmp_path / 'idx.npy'))
    with open(victim, 'ab') as f:                                                  # the size: also caught when the file is read
        f.write(b'\0')
    with pytest.raises(RuntimeError, match='2.jpg'):
        ds[2]
    with pytest.raises(RuntimeError, match='2.jpg'):
        ds.index.check(str(tmp_path))


@pytest.mark.parametrize('workers', [0, 2])
def test_workers_read_bytes_and_never_load_the_library(tmp_path, monkeypatch, workers):
    import torch
    from torchdet3d import _native as N
    from torchdet3d.dataloaders import ObjectronFrames, collate_jpeg
    files = _files()
    files['p.jpg'] = C.encode(C.image(24, 40, 9), '420', 90, progressive=True)
    _dataset(str(tmp_path), files)
    ds = ObjectronFrames(str(tmp_path), 'train', decode='device')
    ds.build_index(threads=2)

    def refuse():
        raise AssertionError('the native library was asked for while items were read')
    monkeypatch.setattr(N, 'lib', refuse)                   # (forked workers inherit it)
    monkeypatch.setattr(N, '_lib', None)
    dl = torch.utils.data.DataLoader(ds, batch_size=5, num_workers=workers, collate_fn=collate_jpeg)
    (blob, table, boxes, labels, counts), = list(dl)
    table, blob = table.numpy(), blob.numpy()
    assert list(table[:, 0]) == [0, 1, 2, 3, 4] and list(table[:, 1]) == [0, 0, 0, 0, 1]
    for k, (name, data) in enumerate(files.items()):
        o = int(table[k, 2])
        if table[k, 1] == 0:
            assert table[k, 3] == len(data) and blob[o:o + len(data)].tobytes() == data
        else:                                               # the progressive file: the host-decoded frame
            assert tuple(table[k, 3:]) == (24, 40)
            assert np.array_equal(blob[o:o + 24 * 40 * 3].reshape(24, 40, 3), C.pillow(data))
    assert boxes.shape == (5, 4) and list(counts) == [1] * 5
