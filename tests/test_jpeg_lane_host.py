"""CPU: the code one lane of the device JPEG decode runs (csrc/jpeg_decode.h), compiled for the host.  tools/jpeg_index_check.cpp
walks it over the matrix of tests/jpeg_cases.py and over the truncations and mutations test_jpeg_host.py gives the indexer: every
file the indexer accepts decodes, whole and rectangle by rectangle, with every seg_mcus to the same pixels, inside buffers of
exactly the sizes the entry points are given.  The rectangles are compared with the tool's own whole-frame decode, which runs the
same parser, so the whole frames of the matrix are also held to Pillow's pixels here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_lane_code_decodes_every_accepted_file_whole_and_by_rectangles(tmp_path):
    from torchdet3d.dataloaders import jpeg as J
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    files = C.malformed()[1] + [d for _, d in C.matrix()]
    C.write_files(str(tmp_path / 'corpus'), files)
    tool = str(tmp_path / 'jpeg_index_check')
    subprocess.run([cxx, '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'jpeg_index_check.cpp'), '-o', tool], check=True)
    r = subprocess.run([tool, str(tmp_path / 'corpus'), '--dump'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r'(\d+) files: (\d+) accepted and decoded, \d+ malformed, \d+ unsupported, (\d+) rectangles compared, (\d+) findings',
                  r.stdout)
    assert m, r.stdout[-2000:]
    n, accepted, rects, findings = (int(v) for v in m.groups())
    assert findings == 0 and n == len(files)
    assert accepted == sum(J.index_jpeg(d, 1)[0] == 0 for d in files)
    assert rects > 0
    first = len(C.malformed()[1])                       # (the matrix follows the malformed files)
    for k, (name, data) in enumerate(C.matrix()):
        rgb = np.fromfile(str(tmp_path / 'corpus' / f'{first + k:04d}.jpg.rgb'), np.uint8)
        want = C.pillow(data)
        assert rgb.size == want.size and np.array_equal(rgb.reshape(want.shape), want), name
