"""CPU: the code one lane of the device JPEG indexer runs (csrc/jpeg_scan.h), compiled for the host, and the marker half of the
host indexer (t3d_jpeg_header).  tools/jpeg_scan_check.cpp runs the passes of t3d_jpeg_index_device lane by lane -- speculate,
settle rounds to the fixed point, count, emit -- over the matrix of tests/jpeg_cases.py and the truncations and mutations
test_jpeg_host.py gives the indexer, for seg_mcus 1, 2, 3 and one segment per image and three lane sizes.  The yardstick is the
host indexer: accept / refuse equals its for every file, and every accepted file's rows and scan_bytes are equal."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as C
import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_LANE = 1 << 20                      # larger than any scan of the corpus


def _J():
    from torchdet3d.dataloaders import jpeg as J
    return J


def _noise():
    """64 x 64 uniform noise at quality 100, 4:4:4: full blocks, stuffed bytes, long extra bits."""
    return C.encode(np.random.default_rng(7).integers(0, 256, (64, 64, 3), dtype=np.uint8), '444', 100)


def _extras():
    """(a file with 1 KB of arbitrary bytes behind EOI, two files concatenated, the noise image): the host accepts all three."""
    base = C.matrix()[200][1]
    tail = bytes(np.random.default_rng(3).integers(0, 256, 1024, dtype=np.uint8))
    return [base + tail, base + C.matrix()[100][1], _noise()]


def _symbols(data):
    """The symbols of an accepted file's scan, walked with the numpy restatement's reader: [(first bit, first extra bit, end bit,
    block number)] in bits of the UNSTUFFED scan, and the reader (its `at` maps a stuffed offset to a bit)."""
    p = R.parse(data)
    f = 2 if p['sampling'] == R.S420 else 1
    nmcu = -(-p['w'] // (8 * f)) * -(-p['h'] // (8 * f))
    br = R._Bits(bytes(data)[p['scan']:])
    out, block = [], 0
    for _ in range(nmcu):
        for c in range(p['ncomp']):
            for _ in range(f * f if c == 0 else 1):
                a = br.p
                t = br.symbol(p['dc'][c])
                b = br.p
                br.get(t)
                out.append((a, b, br.p, block))
                k = 1
                while k < 64:
                    a = br.p
                    rs = br.symbol(p['ac'][c])
                    b = br.p
                    r, s = rs >> 4, rs & 15
                    if s == 0 and r != 15:
                        out.append((a, b, b, block))
                        break
                    k += 16 if s == 0 else r + 1
                    br.get(s)
                    out.append((a, b, br.p, block))
                block += 1
    return out, br


def test_the_smallest_lanes_cut_the_corpus_in_every_awkward_place():
    J = _J()
    sub = J.SUB_BYTES_RANGE[0]
    on_stuffed = on_ff = in_extra = twice = 0
    for data in [d for n, d in C.matrix() if n.startswith('40x56')] + [_noise()]:
        rc, info, _ = J.index_jpeg(data, 1)
        assert rc == 0
        scan = np.frombuffer(data, np.uint8)[int(info['scan_offset']):][:int(info['scan_bytes'])]
        cuts = np.arange(sub, scan.size - 1, sub)                         # the first byte of every lane but lane 0
        on_stuffed += int(((scan[cuts] == 0) & (scan[cuts - 1] == 0xFF)).sum())
        on_ff += int(((scan[cuts] == 0xFF) & (scan[cuts + 1] == 0)).sum())
        syms, br = _symbols(data)
        s = np.array(syms, np.int64)
        cut_bits = np.array([br.at[c] for c in cuts.tolist() if c in br.at], np.int64)      # (a cut on a stuffed 00 lies between two bytes)
        cut_bits = cut_bits[cut_bits < s[-1, 2]]                            # (not those in the padding behind the last symbol)
        k = np.searchsorted(s[:, 0], cut_bits, side='right') - 1            # the symbol each cut lies in (or begins)
        in_extra += int(((cut_bits > s[k, 1]) & (cut_bits < s[k, 2])).sum())
        inside = cut_bits != s[k, 0]                                        # cuts strictly inside a symbol or between two of one block
        first_of_block = np.concatenate([[True], s[1:, 3] != s[:-1, 3]])
        interior = ~(first_of_block[k] & ~inside)                           # not exactly on a block's first bit
        twice += int((np.bincount(s[k[interior], 3]) >= 2).sum())
    assert on_stuffed >= 1 and on_ff >= 1 and in_extra >= 1 and twice >= 1, (on_stuffed, on_ff, in_extra, twice)


def test_the_lanes_index_every_file_as_the_host_indexer_does(tmp_path):
    J = _J()
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    corpus = C.malformed()[1]
    assert len(corpus) == 1098 and sum(J.index_jpeg(d, 1)[0] == 0 for d in corpus) == 149
    files = corpus + [d for _, d in C.matrix()] + _extras()
    want = [J.index_jpeg(d, 1)[0] == 0 for d in files]
    assert all(want[len(corpus):])                      # the matrix, the file with a tail and the concatenated pair are accepted
    C.write_files(str(tmp_path / 'corpus'), files)
    tool = str(tmp_path / 'jpeg_scan_check')
    subprocess.run([cxx, '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'jpeg_scan_check.cpp'), '-o', tool], check=True)
    subs = [J.SUB_BYTES_RANGE[0], J.DEFAULT_SUB_BYTES, ONE_LANE]
    r = subprocess.run([tool, str(tmp_path / 'corpus')] + [str(s) for s in subs], capture_output=True, text=True)
    tail = '\n'.join(l for l in r.stdout.splitlines() if ' settle rounds, ' not in l)[-3000:]
    assert r.returncode == 0, tail + r.stderr[-2000:]
    m = re.search(r'(\d+) files: (\d+) accepted, (\d+) refused by the scan, (\d+) refused by the markers, (\d+) runs compared, '
                  r'most settle rounds (\d+), (\d+) findings', r.stdout)
    assert m, tail
    n, accepted, by_scan, by_markers, runs, _, findings = (int(v) for v in m.groups())
    assert findings == 0 and n == len(files)            # no file is left out
    assert accepted == sum(want) and by_scan + by_markers == len(files) - sum(want)
    assert runs == (accepted + by_scan) * 4 * len(subs)
    # one line per file and lane size: every file went through every lane size, and one lane settles in no round at all
    lines = re.findall(r'^(\d+)\.jpg sub_bytes (\d+): status (\d), (\d+) settle rounds, (\d+) lanes$', r.stdout, re.M)
    assert len(lines) == (accepted + by_scan) * len(subs)
    for name, sub, status, rounds, lanes in lines:
        assert (int(status) == 0) == want[int(name)]
        assert int(rounds) <= max(int(lanes) - 1, 0) or int(lanes) == 0
        if int(sub) == ONE_LANE:
            assert int(lanes) <= 1 and int(rounds) == 0


def _sixteen_bit_table(data):
    """A baseline file whose first DQT is rewritten with 16-bit entries."""
    at = data.index(b'\xff\xdb')
    n = (data[at + 2] << 8) | data[at + 3]
    assert n == 67                                      # (Pillow writes one table a segment)
    wide = b''.join(bytes([0, v]) for v in data[at + 5:at + 69])
    return data[:at] + b'\xff\xdb' + (131).to_bytes(2, 'big') + bytes([0x10 | data[at + 4]]) + wide + data[at + 69:]


def test_the_header_is_the_marker_half_of_the_indexer():
    import io

    from PIL import Image
    J = _J()
    for name, data in C.matrix():
        rc, want, _ = J.index_jpeg(data, 3)
        rh, got = J.read_jpeg_header(data, 3)
        assert rc == 0 and rh == 0, name
        assert int(got['scan_bytes']) == len(data) - int(want['scan_offset']), name
        got = got.copy()
        got['scan_bytes'] = want['scan_bytes']
        assert got.tobytes() == want.tobytes(), name
    img = C.image(24, 40, 1)
    cmyk = io.BytesIO()
    Image.fromarray(np.concatenate([img, img[..., :1]], -1), 'CMYK').save(cmyk, format='JPEG', quality=90)
    base = C.encode(img, '420', 90)
    files = {'progressive': (C.encode(img, '420', 90, progressive=True), 1), '4:2:2': (C.encode(img, '422', 90), 4),
             'restart markers': (C.encode(img, '420', 90, restart_marker_rows=1), 3), 'CMYK': (cmyk.getvalue(), 5),
             '16-bit table': (_sixteen_bit_table(base), 7)}
    from torchdet3d import _native as N
    for name, (data, reason) in files.items():
        rc, want, _ = J.index_jpeg(data)
        rh, got = J.read_jpeg_header(data)
        assert rc == rh == N.ERR_UNSUPPORTED and int(got['reason']) == int(want['reason']) == reason, name
        assert got.tobytes() == want.tobytes(), name
    scan_at = int(J.index_jpeg(base)[1]['scan_offset'])
    for n in range(scan_at + 1):                        # every header truncation (at scan_at the markers are whole)
        rc, want, _ = J.index_jpeg(base[:n])
        rh, got = J.read_jpeg_header(base[:n])
        if n < scan_at:
            assert rh == rc != 0 and got.tobytes() == want.tobytes(), n
        else:
            assert rh == 0 and rc == N.ERR_ARG and int(got['scan_bytes']) == 0, n


def test_argument_errors_come_before_any_gpu_call():
    from torchdet3d import _native as N
    J = _J()
    lib = N.lib()
    nbytes = ctypes.c_longlong(-1)
    assert lib.t3d_jpeg_index_work_bytes(1000, 2, 64, ctypes.byref(nbytes)) == 0 and nbytes.value == (2 * 2 + 1000 // 64) * 32
    lo, hi = J.SUB_BYTES_RANGE
    assert lo <= 8
    for args in ((1000, 2, 64, None), (-1, 2, 64, ctypes.byref(nbytes)), (1000, -1, 64, ctypes.byref(nbytes)),
                 (1000, 65536, 64, ctypes.byref(nbytes)), (1000, 2, lo - 1, ctypes.byref(nbytes)), (1000, 2, hi + 1, ctypes.byref(nbytes))):
        assert lib.t3d_jpeg_index_work_bytes(*args) == N.ERR_ARG, args
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data % 16)       # (host memory: no argument error may get as far as a launch)
    good = dict(data=p, data_bytes=100, infos=p, segs=p, total_segs=4, items=p, sub_bytes=64, work=p, work_bytes=1024, status=p, B=1,
                max_subs=1, stream=None)
    bad = [dict(data=None), dict(infos=None), dict(segs=None), dict(items=None), dict(work=None), dict(status=None), dict(B=-1),
           dict(B=65536), dict(sub_bytes=lo - 1), dict(sub_bytes=hi + 1), dict(work=p + 8), dict(work_bytes=31), dict(data_bytes=0),
           dict(total_segs=0), dict(max_subs=0)]
    for change in bad:
        assert lib.t3d_jpeg_index_device(*{**good, **change}.values()) == N.ERR_ARG, change
    assert lib.t3d_jpeg_index_device(*{**good, 'B': 0, 'data': None}.values()) == 0      # B == 0: nothing else is looked at
    info = np.zeros(1, J.INFO_DTYPE)
    data = np.frombuffer(C.matrix()[0][1], np.uint8)
    assert lib.t3d_jpeg_header(None, 10, 2, info.ctypes.data) == N.ERR_ARG
    assert lib.t3d_jpeg_header(data.ctypes.data, data.size, 2, None) == N.ERR_ARG
    assert lib.t3d_jpeg_header(data.ctypes.data, data.size, 0, info.ctypes.data) == N.ERR_ARG
    assert lib.t3d_jpeg_header(data.ctypes.data, -1, 2, info.ctypes.data) == N.ERR_ARG


def test_a_device_build_without_a_gpu_says_so(tmp_path, monkeypatch):
    import torch
    J = _J()
    with pytest.raises(ValueError, match="'host' or 'device'"):
        J.JpegIndex.build([], str(tmp_path), where='gpu')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # (where there is one, tests/test_gpu_jpeg_index.py builds on it)
    with open(tmp_path / 'a.jpg', 'wb') as f:
        f.write(C.matrix()[0][1])
    with pytest.raises(RuntimeError, match='needs a GPU'):
        J.JpegIndex.build(['a.jpg'], str(tmp_path), where='device')
