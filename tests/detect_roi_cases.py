"""The inputs `t3d_detect_roi_plan_host` is held to numpy over (tests/test_detect_roi_plan_host.py) and `t3d_detect_roi_plan` to
`t3d_detect_roi_plan_host` (tests/test_gpu_detection_arena_crop.py): per case of tests/detect_draw_cases.py the records
`t3d_detect_draw_host` makes at B = 12 and hand-made ones behind them, the index rows of a Pillow-encoded file of the case's size
per sampling and seg_mcus, and whole-frame items as a batch of such frames would have them."""
import numpy as np

import detect_draw_cases as K
import jpeg_cases as C

B = 12
SAMPLINGS = ('420', '444', 'gray')
SEG_MCUS = (1, 2, 3)
INT_MAX = 2 ** 31 - 1
PER_TURN = 11                    # hand-made records per turn


def hand_made(base, h, w, offset):
    """Records that force what the draws only reach by chance: per turn, with an Expand paste, the crop equal to the canvas, two
    crops wholly in the fill, a crop inside the frame, one across its corner, one pixel at each corner of the pasted frame; a
    negative paste; a paste at the end of the integers, where the shifted position saturates."""
    out = []

    def add(turns, left, top, crop, flags=0):
        r = base.copy()
        r['offset'], r['h'], r['w'], r['turns'], r['left'], r['top'], r['flags'] = offset, h, w, turns, left, top, flags
        r['cx0'], r['cy0'], r['cx1'], r['cy1'] = crop
        out.append(r)
    for t in (0, 1, 3):
        rw, rh = (w, h) if t == 0 else (h, w)
        l, tp = 37, 21
        W, H = 2 * rw + 50, 2 * rh + 40
        add(t, l, tp, (0, 0, W, H))
        add(t, l, tp, (0, 0, l, tp), 1)
        add(t, l, tp, (l + rw, 3, W, H - 2))
        add(t, l, tp, (l + 5, tp + 7, l + rw - 3, tp + rh - 5), 1)
        add(t, l, tp, (l - 10, tp - 4, l + 9, tp + 11))
        add(t, l, tp, (l - 3, tp - 2, l + 1, tp + 1))
        add(t, l, tp, (l + rw - 1, tp - 2, l + rw + 5, tp + 1), 1)
        add(t, l, tp, (l - 3, tp + rh - 1, l + 1, tp + rh + 4))
        add(t, l, tp, (l + rw - 1, tp + rh - 1, l + rw + 2, tp + rh + 2))
        add(t, -6, -3, (0, 0, rw - 8, rh - 4))
        add(t, INT_MAX - 2, INT_MAX - 1, (5, 6, 40, 50))
    assert len(out) == 3 * PER_TURN
    return np.array(out, base.dtype)


_rows = {}


def index_rows(h, w, sampling, seg_mcus):
    """(file bytes, info, segs) of a Pillow-encoded file of this size, made once."""
    from torchdet3d.dataloaders import jpeg as J
    if (h, w, sampling) not in _rows:
        _rows[h, w, sampling] = C.encode(C.image(h, w, h + w), sampling, 90)
    key = (h, w, sampling, seg_mcus)
    if key not in _rows:
        rc, info, segs = J.index_jpeg(_rows[h, w, sampling], seg_mcus)
        assert rc == 0 and (int(info['h']), int(info['w'])) == (h, w)
        _rows[key] = (_rows[h, w, sampling], info, segs)
    return _rows[key]


_drawn = None


def drawn():
    """{case name: (case, records [B + hand-made], src_bytes)} -- the draws computed once."""
    global _drawn
    if _drawn is None:
        from torchdet3d.dataloaders.detection_arena import detect_draw_host
        _drawn = {}
        for case in K.cases():
            frames, boxes, labels, start = K.tables(case, B)
            rec = detect_draw_host(K.pipeline(case), case['key'], frames, boxes, labels, start, case['G'])[0]
            nb = case['h'] * case['w'] * 3
            more = hand_made(rec[0], case['h'], case['w'], 0)
            more['offset'] = (B + np.arange(len(more))) * nb
            _drawn[case['name']] = (case, np.concatenate([rec, more]), (B + len(more)) * nb)
    return _drawn


def whole_items(n, info, file_bytes):
    """The t3d_jpeg_item table of n whole frames of this file, one behind the other, somewhere in resident tables."""
    from torchdet3d.dataloaders import jpeg as J
    blocks = np.full(n, int(J.frame_blocks(np.array([info]))[0]), np.int64)
    nb = int(info['h']) * int(info['w']) * 3
    return J.item_table(1000 + np.arange(n) * (file_bytes + 7), file_bytes, np.arange(n) * nb, 5 + np.arange(n) * int(info['nseg']), blocks)
