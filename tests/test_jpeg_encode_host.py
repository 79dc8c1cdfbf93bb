"""CPU: the JPEG encoder's definition and its host half.  The numpy restatement tests/jpeg_encode_ref.py writes Pillow's files
byte for byte (Pillow on libjpeg-turbo -- asserted, not skipped on); `t3d_jpeg_encode_setup` writes the restatement's header,
divisors and code tables; the argument refusals of the two host calls; `index_jpeg` accepts the files; and the code ONE LANE of
every kernel runs (csrc/jpeg_encode.h), compiled for the host and run lane by lane by tools/jpeg_encode_check.cpp, writes the
restatement's files too -- dummy blocks, segment cuts, the overflow rows and the untouched slot of a frame that does not fit."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import features

import jpeg_encode_cases as C
import jpeg_encode_ref as R
from conftest import ROOT


@pytest.fixture(scope='module')
def N():
    from torchdet3d import _native
    assert os.path.exists(_native.LIB_PATH), 'run `python __graft_entry__.py` (build()) first'
    return _native


# ---- 1. the restatement is Pillow's encoder ------------------------------------------------------------------------------------------
def test_pillow_is_libjpeg_turbo():
    assert features.check_feature('libjpeg_turbo'), 'byte parity is pinned against Pillow on libjpeg-turbo'


@pytest.mark.parametrize('h,w', C.SIZES)
def test_restatement_writes_pillows_file(h, w):
    assert features.check_feature('libjpeg_turbo')
    for name, frame in (('noise', C.noise(h, w)), ('smooth', C.smooth(h, w))):
        for q in C.QUALITIES:
            for s in C.SAMPLINGS:
                assert R.encode(frame, q, s) == C.pillow(frame, q, s), (name, h, w, q, s)


def test_restatement_writes_pillows_file_for_the_extreme_contents():
    assert features.check_feature('libjpeg_turbo')
    for name, frame in C.extremes():
        for q in C.QUALITIES:
            for s in C.SAMPLINGS:
                assert R.encode(frame, q, s) == C.pillow(frame, q, s), (name, q, s)


def test_the_fixed_header_form():
    hd = R.header(270, 480, 90, 2)
    assert len(hd) == 623 and hd[:20] == bytes.fromhex('ffd8ffe000104a46494600010100000100010000')
    assert hd[20:25] == bytes.fromhex('ffdb004300') and hd[89:94] == bytes.fromhex('ffdb004301')
    assert hd[158:177] == bytes.fromhex('ffc000110801 0e01e0 03 012200 021101 031101'.replace(' ', ''))
    assert [hd[i + 3] for i in (177, 210, 393, 426)] == [0x1F, 0xB5, 0x1F, 0xB5] and [hd[i + 4] for i in (177, 210, 393, 426)] == [0, 0x10, 1, 0x11]
    assert hd[-14:] == bytes.fromhex('ffda000c03010002110311003f00')
    assert R.header(8, 8, 90, 1)[158 + 11] == 0x11


# ---- 2. t3d_jpeg_encode_setup -----------------------------------------------------------------------------------------------------
def test_setup_writes_the_restatements_header_divisors_and_codes(N):
    from torchdet3d.utils.jpeg_encode import ENC_TABLES_DTYPE, encode_tables
    assert ENC_TABLES_DTYPE.itemsize == 5040
    codes = [R.huff_codes(R.DC_BITS[0], R.DC_VALS[0]), R.huff_codes(R.DC_BITS[1], R.DC_VALS[1]),
             R.huff_codes(R.AC_BITS[0], R.AC_VALS[0]), R.huff_codes(R.AC_BITS[1], R.AC_VALS[1])]
    want_huff = np.stack([(size << 16) | code for code, size in codes]).astype(np.uint32)
    for h, w in ((1, 1), (8, 8), (33, 17), (65535, 1)):
        for s in (1, 2):
            for q in range(1, 101):
                rc, t = encode_tables(h, w, q, s)
                assert rc == 0
                t = t[0]
                n = int(t['header_bytes'])
                assert bytes(t['header'][:n]) == R.header(h, w, q, s), (h, w, q, s)
                assert not t['header'][n:].any()
                ql, qc = R.quant_tables(q)
                assert np.array_equal(t['divisor'], np.stack([8 * ql, 8 * qc])), (q,)
                assert np.array_equal(t['huff'], want_huff)
                px = 16 if s == 2 else 8
                assert (int(t['h']), int(t['w']), int(t['quality']), int(t['sampling'])) == (h, w, q, s)
                assert (int(t['mcus_x']), int(t['mcus_y']), int(t['mcu_blocks'])) == (-(-w // px), -(-h // px), 6 if s == 2 else 3)
                assert int(t['blocks']) == int(t['mcus_x']) * int(t['mcus_y']) * int(t['mcu_blocks'])
                assert (int(t['luma_rows']), int(t['luma_cols'])) == (-(-h // 8), -(-w // 8))
    assert encode_tables(8, 8, 90, '420')[1]['sampling'][0] == 2 and encode_tables(8, 8, 90, '444')[1]['sampling'][0] == 1


def test_setup_and_work_bytes_refuse_bad_arguments(N):
    from torchdet3d.utils.jpeg_encode import ENC_TABLES_DTYPE
    lib = N.lib()
    t = np.full(ENC_TABLES_DTYPE.itemsize, 0x5A, np.uint8)
    for h, w, q, s in ((0, 8, 90, 2), (8, 0, 90, 2), (65536, 8, 90, 2), (8, 65536, 90, 1), (-1, 8, 90, 2), (8, 8, 0, 2), (8, 8, 101, 1),
                       (8, 8, 90, 0), (8, 8, 90, 3)):
        assert lib.t3d_jpeg_encode_setup(h, w, q, s, t.ctypes.data) == N.ERR_ARG, (h, w, q, s)
        assert (t == 0x5A).all(), 'a refused call wrote to the struct'
    assert lib.t3d_jpeg_encode_setup(8, 8, 90, 2, None) == N.ERR_ARG
    assert lib.t3d_jpeg_encode_setup(65535, 65535, 100, 1, t.ctypes.data) == 0
    nb = ctypes.c_longlong(-7)
    ok = (2, 33, 17, 2, 3, 4096)
    assert lib.t3d_jpeg_encode_work_bytes(*ok, ctypes.byref(nb)) == 0
    # coefficients, segment offsets, the unstuffed streams, the FF counts: 36 blocks, 2 segments and 64 chunks a frame
    assert nb.value == 2 * 36 * 128 + 48 + 2 * 4096 + 528 and nb.value % 16 == 0
    assert lib.t3d_jpeg_encode_work_bytes(0, 33, 17, 2, 3, 4096, ctypes.byref(nb)) == 0 and nb.value == 0
    assert lib.t3d_jpeg_encode_work_bytes(*ok, None) == N.ERR_ARG
    for i, v in ((0, -1), (0, 65536), (1, 0), (1, 65536), (2, 0), (2, 65536), (3, 0), (3, 3), (4, 0), (5, 624), (5, (1 << 40) + 1)):
        args = list(ok)
        args[i] = v
        nb.value = -7
        assert lib.t3d_jpeg_encode_work_bytes(*args, ctypes.byref(nb)) == N.ERR_ARG, (i, v)
        assert nb.value == -7
    assert lib.t3d_jpeg_encode_work_bytes(2, 33, 17, 2, 3, 625, ctypes.byref(nb)) == 0


def test_b_zero_and_refusals_of_the_encode_call_need_no_gpu(N):
    """B == 0 returns at once; every T3D_ERR_ARG is decided before anything is launched (no GPU here, so nothing can be)."""
    from torchdet3d.utils.jpeg_encode import encode_tables
    lib = N.lib()
    _, t = encode_tables(33, 17, 90, 2)
    nb = ctypes.c_longlong(0)
    assert lib.t3d_jpeg_encode_work_bytes(2, 33, 17, 2, 2, 4096, ctypes.byref(nb)) == 0
    good = [4096, 2, t.ctypes.data, 8192, 2, 4096 * 3, 4096, 4096 * 5, 4096 * 7, nb.value, None]      # (addresses nobody reads)
    assert lib.t3d_jpeg_encode_u8(None, 0, None, None, 0, None, 0, None, None, 0, None) == 0
    for i, v in ((0, None), (1, -1), (1, 65536), (2, None), (3, None), (4, 0), (5, None), (5, 4096 * 3 + 8), (6, 624), (7, None),
                 (8, None), (8, 4096 * 7 + 4), (9, nb.value - 1)):
        args = list(good)
        args[i] = v
        assert lib.t3d_jpeg_encode_u8(*args) == N.ERR_ARG, (i, v)
    bad = t.copy()
    bad['mcus_x'] += 1                                    # tables that setup does not write
    args = list(good)
    args[2] = bad.ctypes.data
    assert lib.t3d_jpeg_encode_u8(*args) == N.ERR_ARG


# ---- 3. the project's own index takes the files -------------------------------------------------------------------------------------
def test_index_accepts_the_restatements_files(N):
    from torchdet3d.dataloaders.jpeg import index_jpeg
    for h, w in C.SIZES[:4]:
        for s in C.SAMPLINGS:
            for q in (1, 90, 100):
                rc, info, segs = index_jpeg(R.encode(C.noise(h, w), q, s), 2)
                assert rc == 0 and int(info['reason']) == 0, (h, w, s, q)
                assert (int(info['sampling']), int(info['h']), int(info['w'])) == (s, h, w)
                assert len(segs) == int(info['nseg']) == -(-int(info['mcus_x']) * int(info['mcus_y']) // 2)


# ---- 4. the lane code of the kernels, on the host -------------------------------------------------------------------------------------
def test_the_lane_code_writes_the_restatements_files(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'a host C++ compiler'
    tool = str(tmp_path / 'jpeg_encode_check')
    subprocess.run([cxx, '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'jpeg_encode_check.cpp'), '-o', tool], check=True)
    corpus = tmp_path / 'corpus'
    corpus.mkdir()
    cases = []
    for k, ((h, w), q, s, seg) in enumerate([((8, 8), 100, 2, 1), ((16, 16), 50, 1, 2), ((33, 17), 90, 2, 3), ((33, 17), 1, 1, 7),
                                             ((40, 56), 100, 2, 2), ((40, 56), 90, 1, 1000), ((100, 130), 90, 2, 2)]):
        frames = np.stack([C.noise(h, w), C.smooth(h, w), C.checker(h, w)])
        want = [R.encode(f, q, s) for f in frames]
        cases.append((f'{h}_{w}_{q}_{s}_{seg}_3_{max(len(x) for x in want)}_case{k}', frames, q, s, want))
    ext = np.stack([f for _, f in C.extremes()])
    for s in C.SAMPLINGS:
        want = [R.encode(f, 100, s) for f in ext]
        cases.append((f'24_40_100_{s}_2_6_{max(len(x) for x in want) + 5}_extreme{s}', ext, 100, s, want))
    # a slot only the smallest file fits; and one in which only the STUFFED file of frame 1 does not fit
    frames = np.stack([C.noise(40, 56, i) for i in range(3)])
    want = [R.encode(f, 100, 1) for f in frames]
    cases.append((f'40_56_100_1_2_3_{min(len(x) for x in want)}_small', frames, 100, 1, want))
    cases.append((f'40_56_100_1_2_3_{623 + R.unstuffed_scan_bytes(frames[1], 100, 1) + 2 + 64}_stuffed', frames, 100, 1, want))
    # and a slot far smaller than the middle frame's SCAN: that frame's emit, FF count and scatter lanes do not run
    mixed = np.stack([C.smooth(40, 56), frames[1], C.smooth(40, 56)[::-1].copy()])
    want = [R.encode(f, 100, 1) for f in mixed]
    cases.append((f'40_56_100_1_2_3_{max(len(want[0]), len(want[2]))}_scan', mixed, 100, 1, want))
    assert max(len(want[0]), len(want[2])) + 64 < R.unstuffed_scan_bytes(mixed[1], 100, 1)
    for name, frames, *_ in cases:
        frames.tofile(str(corpus / (name + '.rgb')))
    r = subprocess.run([tool, str(corpus)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name, frames, q, s, want in cases:
        B, cap = len(frames), int(name.split('_')[6])
        raw = np.fromfile(str(corpus / (name + '.out')), np.uint8)
        res, out = raw[:16 * B].view(np.dtype([('bytes', '<i8'), ('overflow', '<i4'), ('reserved', '<i4')])), raw[16 * B:].reshape(B, cap)
        for i in range(B):
            if len(want[i]) <= cap:
                assert (int(res['bytes'][i]), int(res['overflow'][i])) == (len(want[i]), 0), (name, i)
                assert out[i, :len(want[i])].tobytes() == want[i], (name, i)
                assert (out[i, len(want[i]):] == 0xEE).all(), (name, i)
            else:
                assert int(res['overflow'][i]) == 1 and (out[i] == 0xEE).all(), (name, i)
                assert int(res['bytes'][i]) == 623 + R.unstuffed_scan_bytes(frames[i], q, s) + 2, (name, i)
    assert any(len(x) > int(n.split('_')[6]) for n, _, _, _, w in cases for x in w), 'no overflowing frame among the cases'
