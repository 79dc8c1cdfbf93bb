"""GPU: `t3d_detect_draw` (csrc/detect_draw.hip) equals `t3d_detect_draw_host` -- the same header on the CPU, which
tests/test_detect_draw_host.py holds to numpy -- byte for byte over the cases of tests/detect_draw_cases.py, in batched calls of
B = 1 and B = 67, every output in a buffer with guard bytes on both sides; bad rows; argument errors launch nothing."""
import numpy as np
import pytest
import torch

import detect_draw_cases as K

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5


def _device(case, B, frames, boxes, labels, start, G):
    """One t3d_detect_draw call -> (records, gt_boxes, gt_labels, gt_counts, diag as numpy, guards untouched)."""
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.detection import DET_SAMPLE_DTYPE
    from torchdet3d.dataloaders.detection_arena import key_words, pipeline_cfg
    cfg, words = pipeline_cfg(K.pipeline(case)), key_words(case['key'])
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (frames, boxes, labels, start)]
    sizes = [B * 80, B * G * 16, B * G * 4, B * 4, B * 8]
    outs = [torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda') for n in sizes]
    N.call('t3d_detect_draw', cfg.ctypes.data, len(cfg), words.ctypes.data, len(words), N.ptr(d[0]), B, N.ptr(d[1]), N.ptr(d[2]),
           N.ptr(d[3]), len(start) - 1, len(labels), G, *[o.data_ptr() + GUARD for o in outs], N.stream())
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    clean = all(np.all(h[:GUARD] == FILL) and np.all(h[GUARD + n:] == FILL) for h, n in zip(host, sizes))
    body = [h[GUARD:GUARD + n].copy() for h, n in zip(host, sizes)]
    return (body[0].view(DET_SAMPLE_DTYPE), body[1].view(np.float32).reshape(B, G, 4), body[2].view(np.int32).reshape(B, G),
            body[3].view(np.int32), body[4].view(np.int32).reshape(B, 2)), clean


def _same(got, want, what):
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes(), what


@pytest.mark.parametrize('B', [1, 67])
def test_the_device_equals_the_host_entry_over_the_case_list(B):
    from torchdet3d.dataloaders.detection_arena import detect_draw_host
    for case in K.cases():
        t = K.tables(case, B)
        got, clean = _device(case, B, *t, case['G'])
        assert clean, f'{case["name"]}: a byte outside the outputs was written'
        _same(got, detect_draw_host(K.pipeline(case), case['key'], *t, case['G']), case['name'])


def test_bad_rows_give_zero_records_and_leave_the_neighbours_alone():
    from torchdet3d.dataloaders.detection_arena import detect_draw_host
    case = K.cases()[3]                                         # three images, the middle one at capacity
    frames, boxes, labels, start = K.tables(case, 6)
    good, _ = _device(case, 6, frames, boxes, labels, start, case['G'])
    bad = frames.copy()
    bad[1, 3], bad[4, 3] = 3, -1                                # indices outside the table
    got, clean = _device(case, 6, bad, boxes, labels, start, case['G'])
    assert clean
    for k in (1, 4):
        assert not got[0][k:k + 1].tobytes().strip(b'\0') and got[3][k] == 0 and not got[1][k].view(np.uint32).any() and not got[2][k].any()
    for k in (0, 2, 3, 5):
        _same([g[k] for g in got], [g[k] for g in good], k)
    short = start.copy()
    short[2] = len(labels) + 1                                  # image 1's box range runs behind the table (and image 2's is negative)
    got, clean = _device(case, 6, frames, boxes, labels, short, case['G'])
    assert clean and list(got[3] > 0) == [True, False, False, True, False, False]
    _same(got, detect_draw_host(K.pipeline(case), case['key'], frames, boxes, labels, short, case['G']), 'box range')
    _same([g[0] for g in got], [g[0] for g in good], 0)


def test_argument_errors_launch_nothing():
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.detection_arena import key_words, pipeline_cfg
    case = K.cases()[1]
    frames, boxes, labels, start = K.tables(case, 2)
    cfg, words = pipeline_cfg(K.pipeline(case)), key_words(case['key'])
    d = [torch.from_numpy(a).cuda() for a in (frames, boxes, labels, start)]
    outs = [torch.zeros(n, dtype=torch.uint8, device='cuda') for n in (160, 32, 8, 8, 16)]
    good = [cfg.ctypes.data, len(cfg), words.ctypes.data, len(words), N.ptr(d[0]), 2, N.ptr(d[1]), N.ptr(d[2]), N.ptr(d[3]), 1, 1, 1,
            *[N.ptr(o) for o in outs]]
    fn = N.lib().t3d_detect_draw
    before = N.launch_count()
    for k, v in {0: None, 2: None, 4: None, 6: None, 7: None, 8: None, 12: None, 13: None, 14: None, 15: None, 16: None, 1: 35, 3: 0, 5: -1,
                 11: 0, 9: -1}.items():
        a = list(good)
        a[k] = v
        assert fn(*a, N.stream()) == N.ERR_ARG, k
    a = list(good)
    a[3] = 17                                                   # more than 16 key words
    assert fn(*a, N.stream()) == N.ERR_ARG
    a = list(good)
    a[11] = 65
    assert fn(*a, N.stream()) == N.ERR_ARG
    a = list(good)
    a[5] = 0
    assert fn(*a, N.stream()) == 0                              # B == 0
    assert N.launch_count() == before
    assert fn(*good, N.stream()) == 0 and N.launch_count() == before + 1
    torch.cuda.synchronize()
