"""GPU: `t3d_jpeg_decode_roi_u8` (csrc/jpeg.hip) bit for bit against `t3d_jpeg_decode_u8` and against Pillow's decode, sliced --
ONE batched call per segment length over every size x sampling x two qualities of the matrix and a list of rectangles per file
(the whole image, single pixels, the last row and column, starts on and next to MCU and chroma-parity boundaries, the ragged
edges), with the whole scan and with only the planned byte span uploaded, output slots at odd offsets and guard bytes around
every slot and around the workspace; the span cut short; inconsistent records; and `decode_jpeg_rois` against `collate_crops`."""
import numpy as np
import pytest
import torch

import jpeg_cases as C

pytestmark = pytest.mark.gpu
GUARD, FILL = 61, 0xA5                               # (an odd guard: the slots sit at odd offsets)
SEG_MCUS = [1, 2, 3, 1 << 20]
_cases = None


def rect_list(h, w):
    r = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, w, 1), (0, h - 1, 1, h), (w - 1, h - 1, w, h), (w // 2, h // 2, w // 2 + 1, h // 2 + 1),
         (0, h - 1, w, h), (w - 1, 0, w, h), (w // 2, h // 2, w, h)]
    for a in (7, 8, 9, 15, 16, 17):                 # MCU and chroma-parity boundaries
        if a < w:
            r.append((a, 0, min(w, a + 5), h))
        if a < h:
            r.append((0, a, w, min(h, a + 5)))
        if a < w and a < h:
            r.append((a, a, min(w, a + 11), min(h, a + 10)))
    return list(dict.fromkeys(r))


def cases():
    """[(name, data, rect, Pillow's pixels of the rectangle)]: the q90 and q100-optimised files of the matrix with `rect_list`,
    and one 100 x 130 image per sampling with interior rectangles (whole MCU rows and columns skipped on all four sides)."""
    global _cases
    if _cases is None:
        _cases = []
        files = [(n, d) for n, d in C.matrix() if n.endswith('_q90_0') or n.endswith('_q100_1')]
        files += [(f'100x130_{s}', C.encode(C.image(100, 130, 900 + k), s, 90)) for k, s in enumerate(C.SAMPLINGS)]
        for name, d in files:
            full = C.pillow(d)
            h, w = full.shape[:2]
            rects = rect_list(h, w) + ([(40, 35, 90, 70), (33, 17, 49, 81), (64, 48, 65, 49)] if h == 100 else [])
            _cases += [(name, d, r, full[r[1]:r[3], r[0]:r[2]]) for r in rects]
    return _cases


def run(items, seg_mcus, partial, cut=0, edit=None, out_short=0):
    """One t3d_jpeg_decode_roi_u8 call over items [(data, rect)], FILL in front of and behind every output slot and the
    workspace.  partial: only the planned span is uploaded, less `cut` bytes at its end.  edit(plan): changes the tables before
    they are uploaded.  -> (crops [h, w, 3] per item, status, guards untouched)."""
    from torchdet3d import _native as N
    from torchdet3d.dataloaders import jpeg as J
    index = {}
    rows, plans, spans, parts = [], [], [], []
    for d, r in items:
        if id(d) not in index:
            rc, info, segs = J.index_jpeg(d, seg_mcus)
            assert rc == 0
            index[id(d)] = info, segs
        info, segs = index[id(d)]
        p = J.plan_roi(info, segs, *r)
        first, n = p['span'] if partial else (0, int(info['scan_bytes']))
        n = max(n - cut, 0)
        rows.append((info, segs)), plans.append(p), spans.append((first, n))
        parts.append(np.frombuffer(d, np.uint8)[int(info['scan_offset']) + first:int(info['scan_offset']) + first + n])
    sizes = np.array([a.size for a in parts], np.int64)
    crop = np.array([(r[3] - r[1]) * (r[2] - r[0]) * 3 for _, r in items], np.int64)
    out_off = GUARD + np.cumsum(crop + GUARD) - (crop + GUARD)
    plan = J.plan_roi_batch(rows, plans, np.cumsum(sizes) - sizes, out_off, spans)
    if edit is not None:
        edit(plan)
    data = np.concatenate(parts + [np.zeros(1, np.uint8)])
    dev = [torch.from_numpy(data).cuda()] + [torch.from_numpy(plan[k].reshape(-1).view(np.uint8).copy()).cuda()
                                             for k in ('infos', 'segs', 'items', 'rects')]
    out = torch.full((int(out_off[-1] + crop[-1] + GUARD),), FILL, dtype=torch.uint8, device='cuda')
    nbytes = plan['total_blocks'] * 192
    arena = torch.full((nbytes + 2 * 64,), FILL, dtype=torch.uint8, device='cuda')
    work = arena[64:64 + nbytes]                                               # (16-byte aligned, as the call demands)
    status = torch.full((len(items),), 77, dtype=torch.int32, device='cuda')
    N.call('t3d_jpeg_decode_roi_u8', N.ptr(dev[0]), int(sizes.sum()) or 1, N.ptr(dev[1]), N.ptr(dev[2]), plan['total_segs'], N.ptr(dev[3]),
           N.ptr(dev[4]), N.ptr(out), out.numel() - out_short, work.data_ptr(), nbytes, plan['total_blocks'], N.ptr(status), len(items),
           plan['max_lanes'], plan['max_blocks'], plan['max_runs'], N.stream())
    torch.cuda.synchronize()
    o, a = out.cpu().numpy(), arena.cpu().numpy()
    mask = np.ones(len(o), bool)
    crops = []
    for (_, r), off, n in zip(items, out_off, crop):
        crops.append(o[off:off + n].reshape(r[3] - r[1], r[2] - r[0], 3))
        mask[off:off + n] = False
    clean = bool(np.all(o[mask] == FILL) and np.all(a[:64] == FILL) and np.all(a[64 + nbytes:] == FILL))
    return crops, status.cpu().numpy(), clean


@pytest.mark.parametrize('partial', [False, True])
@pytest.mark.parametrize('seg_mcus', SEG_MCUS)
def test_every_rectangle_equals_pillows_slice(seg_mcus, partial):
    cs = cases()
    assert len(cs) > 1400
    crops, status, clean = run([(d, r) for _, d, r, _ in cs], seg_mcus, partial)
    assert not status.any(), [(cs[i][0], cs[i][2], int(status[i])) for i in np.flatnonzero(status)[:10]]
    assert clean, 'a byte outside the output slots or the workspace was written'
    bad = [(name, r) for (name, _, r, want), got in zip(cs, crops) if not np.array_equal(got, want)]
    assert not bad, (len(bad), bad[:10])


def test_the_whole_image_equals_the_full_decode():
    from test_gpu_jpeg import run as run_full
    first = {}
    for n, d, r, _ in cases():                      # (`rect_list` begins with the whole image)
        first.setdefault(n, (n, d, r))
    picked = [c for n, c in first.items() if '100x130' not in n]
    full, status, clean = run_full([d for _, d, _ in picked], 2)
    assert not status.any() and clean
    crops, status, clean = run([(d, r) for _, d, r in picked], 2, True)
    assert not status.any() and clean and len(picked) == 90
    for (name, _, _), a, b in zip(picked, crops, full):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize('cut', [1, 12])
@pytest.mark.parametrize('seg_mcus', SEG_MCUS)
def test_a_span_cut_short_stays_inside_its_slot(seg_mcus, cut):
    """One byte short of the plan is inside the read-ahead; twelve bytes short takes real data away.  Either way a lane that
    runs out of bytes is fed zeros: status 0 or 1, never 2, and no byte outside the slots or the workspace."""
    cs = cases()
    crops, status, clean = run([(d, r) for _, d, r, _ in cs], seg_mcus, True, cut=cut)
    assert clean and set(np.unique(status)) <= {0, 1}
    if cut == 1:                                     # (a byte of the read-ahead, unless the span ends with the scan)
        assert sum(np.array_equal(g, want) for (_, _, _, want), g in zip(cs, crops)) > len(cs) // 2


def test_inconsistent_records_are_status_2_and_touch_nothing():
    from torchdet3d import _native as N
    d420 = dict(C.matrix())['40x56_420_q90_0']
    d444 = dict(C.matrix())['37x53_444_q90_0']
    want420, want444 = C.pillow(d420), C.pillow(d444)
    items = [(d420, (16, 16, 40, 30)), (d444, (3, 2, 50, 30))] * 4 + [(d420, (0, 0, 56, 40))]

    def edit(plan):
        r, it = plan['rects'], plan['items']
        r[1, 2] = r[1, 0]                            # an empty rectangle
        r[2, 2] = 57                                 # outside the image
        r[3, 1] = -1
        assert r[4, 4] == 0 and r[4, 5] == 0        # x0 = y0 = 16 are even: their chroma taps reach back into MCU 0
        r[4, 4] = 1                                  # an MCU rectangle that misses the halo
        it['block_offset'][5] = plan['total_blocks'] - 1      # work too small for its blocks
        r[6, 8] += 1                                 # the uploaded segments miss the first needed one
        it['reserved'][7] = 1 << 40                  # a span outside the scan
    crops, status, clean = run(items, 2, True, edit=edit, out_short=GUARD + 1)     # (and `out` ends inside the last item's slot)
    assert clean and list(status) == [0, 2, 2, 2, 2, 2, 2, 2, 2]
    assert np.array_equal(crops[0], want420[16:30, 16:40])
    for c in crops[1:]:
        assert (c == FILL).all()
    # the same batch without the edits decodes
    crops, status, clean = run(items, 2, True)
    assert clean and not status.any() and np.array_equal(crops[1], want444[2:30, 3:50]) and np.array_equal(crops[8], want420)
    # argument errors launch nothing; B == 0 is fine
    fn, before = N.lib().t3d_jpeg_decode_roi_u8, N.launch_count()
    t = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    good = [N.ptr(t), 64, N.ptr(t), N.ptr(t), 1, N.ptr(t), N.ptr(t), N.ptr(t), 64, N.ptr(t), 192, 1, N.ptr(t), 1, 1, 1, 1]
    for k, v in {0: None, 2: None, 3: None, 5: None, 6: None, 7: None, 9: None, 12: None, 1: 0, 4: 0, 8: 0, 11: 0, 13: -1, 14: 0, 15: 0,
                 16: 0, 10: 191}.items():
        args = list(good)
        args[k] = v
        assert fn(*args, N.stream()) == -1, k
    args = list(good)
    args[13] = 0
    assert fn(*args, N.stream()) == 0 and N.launch_count() == before


def test_decode_jpeg_rois_is_the_collate_layout():
    from torchdet3d.dataloaders import collate_crops, decode_jpeg_rois, index_jpeg
    picked = cases()[5::97]
    rows = [index_jpeg(d)[1:] for _, d, _, _ in picked]
    for partial in (True, False):
        packed, desc = decode_jpeg_rois([d for _, d, _, _ in picked], rows, [r for _, _, r, _ in picked], partial=partial)
        torch.cuda.synchronize()
        want = collate_crops([(c, np.zeros((9, 2)), 0) for _, _, _, c in picked])
        assert np.array_equal(desc, want[1].numpy()) and np.array_equal(packed.cpu().numpy(), want[0].numpy())
        assert not decode_jpeg_rois.last_status.cpu().numpy().any()
