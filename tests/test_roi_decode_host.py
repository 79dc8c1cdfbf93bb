"""Host: the planning of the rectangle decode (torchdet3d/dataloaders/jpeg.py: roi_mcus, plan_roi) against brute force.  No GPU
is touched.

The brute force marks, pixel by pixel and chroma tap by chroma tap, the MCUs whose blocks the full decode reads for a rectangle
(the upsampling rules of tests/jpeg_ref.py: `upsample420`).  A pixel's taps are (its rows) x (its columns), and a rectangle is
(its pixel rows) x (its pixel columns), so the marked set of a rectangle is (union of its rows' MCU rows) x (union of its
columns' MCU columns): `marked` loops over the pixels as they are, `_Axis` keeps the two unions as bit masks so that EVERY
rectangle of the small images can be walked, and a test holds the one to the other."""
import numpy as np
import pytest

import jpeg_cases as C
import jpeg_ref as R

SAMPLING = {'gray': R.GRAY, '444': R.S444, '420': R.S420}


def small(h, w):
    """Every rectangle is walked for the sizes up to 17 x 33 and for the thin ones (2 x 40, 49 x 2: the dw <= 2 rule); the larger
    sizes get 200 seeded rectangles."""
    return (h <= 17 and w <= 33) or h * w <= 100


def _taps(p, n, sampling, dw):
    """The sample positions -- (plane: 0 luma / 1 chroma, index) -- that pixel row or column p of n reads along one axis.
    jpeg_ref.upsample420: output 2c + v reads sample c and c - 1 (v = 0) or c + 1 (v = 1), clamped to the d = ceil(n / 2) real
    samples; with dw <= 2 (the WIDTH's samples, for either axis) libjpeg replicates and reads sample c alone."""
    if sampling != R.S420:
        return [(0, p)]
    c, d = p >> 1, (n + 1) >> 1
    taps = [(0, p), (1, c)]
    if dw > 2:
        taps.append((1, max(c - 1, 0) if p % 2 == 0 else min(c + 1, d - 1)))
    return taps


def _mcu(tap, sampling):
    plane, i = tap
    return i >> 4 if sampling == R.S420 and plane == 0 else i >> 3      # a 4:2:0 MCU is 16 luma or 8 chroma samples wide


def marked(sampling, h, w, x0, y0, x1, y1):
    """{(my, mx)}: the MCUs the full decode reads a block of for the pixels [x0, x1) x [y0, y1), pixel by pixel."""
    dw, out = (w + 1) >> 1, set()
    for y in range(y0, y1):
        for x in range(x0, x1):
            for ty in _taps(y, h, sampling, dw):
                for tx in _taps(x, w, sampling, dw):
                    if ty[0] == tx[0]:                                  # (a luma row with a luma column, chroma with chroma)
                        out.add((_mcu(ty, sampling), _mcu(tx, sampling)))
    return out


class _Axis:
    """Bit masks of the MCU rows (or columns) each pixel row (column) marks: mask[p]."""

    def __init__(self, n, sampling, dw):
        self.mask = [sum(1 << m for m in {_mcu(t, sampling) for t in _taps(p, n, sampling, dw)}) for p in range(n)]

    def spans(self):
        """(p0, p1, lo, hi) for every 0 <= p0 < p1 <= n: the union of mask[p0:p1] -- which is asserted to be one run of bits,
        MCUs lo .. hi - 1."""
        for p0 in range(len(self.mask)):
            acc = 0
            for p1 in range(p0 + 1, len(self.mask) + 1):
                acc |= self.mask[p1 - 1]
                lo = (acc & -acc).bit_length() - 1
                hi = acc.bit_length()
                assert acc == (1 << hi) - (1 << lo)
                yield p0, p1, lo, hi


def _rects(h, w, seed):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        yield x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))


@pytest.mark.parametrize('sampling', C.SAMPLINGS)
def test_the_mask_walk_marks_what_the_pixel_walk_marks(sampling):
    s = SAMPLING[sampling]
    for h, w in [(5, 3), (7, 4), (17, 33), (37, 53)]:
        dw = (w + 1) >> 1
        rows, cols = _Axis(h, s, dw), _Axis(w, s, dw)
        for x0, y0, x1, y1 in _rects(h, w, 1):
            my = {m for y in range(y0, y1) for m in range(8) if rows.mask[y] >> m & 1}
            mx = {m for x in range(x0, x1) for m in range(8) if cols.mask[x] >> m & 1}
            assert marked(s, h, w, x0, y0, x1, y1) == {(a, b) for a in my for b in mx}


@pytest.mark.parametrize('sampling', C.SAMPLINGS)
def test_the_mcu_rectangle_is_what_brute_force_marks(sampling):
    from torchdet3d.dataloaders.jpeg import roi_mcus
    s = SAMPLING[sampling]
    n = 0
    for h, w in C.SIZES:
        dw = (w + 1) >> 1
        if small(h, w):                          # every rectangle
            ys = list(_Axis(h, s, dw).spans())
            for x0, x1, mx0, mx1 in _Axis(w, s, dw).spans():
                for y0, y1, my0, my1 in ys:
                    assert roi_mcus(s, h, w, x0, y0, x1, y1) == (mx0, my0, mx1, my1), (h, w, x0, y0, x1, y1)
                    n += 1
        else:
            for x0, y0, x1, y1 in _rects(h, w, h * w):
                mx0, my0, mx1, my1 = roi_mcus(s, h, w, x0, y0, x1, y1)
                assert marked(s, h, w, x0, y0, x1, y1) == {(a, b) for a in range(my0, my1) for b in range(mx0, mx1)}, (h, w, x0, y0, x1, y1)
                n += 1
    assert n > 110000
    for bad in [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, 0, 41, 1), (0, 0, 1, 3), (5, 0, 4, 1)]:
        with pytest.raises(ValueError):
            roi_mcus(s, 2, 40, *bad)


_indexed = {}


def _index(k, seg_mcus):
    """The index rows of file k of the matrix for one segment length, made once."""
    from torchdet3d.dataloaders.jpeg import index_jpeg
    if (k, seg_mcus) not in _indexed:
        rc, info, segs = index_jpeg(C.matrix()[k][1], seg_mcus)
        assert rc == 0
        _indexed[k, seg_mcus] = info, segs
    return _indexed[k, seg_mcus]


@pytest.mark.parametrize('seg_mcus', [1, 2, 3, 1 << 20])
def test_segments_and_byte_span_of_every_rectangle(seg_mcus):
    """For every size x sampling (the q90 file of the matrix): every rectangle of the small images and 200 seeded ones of the
    larger -- the planned segments are the owners of the marked MCUs, each once, and the byte span holds each needed segment
    from its indexed byte up to the indexed byte of the segment behind it (or the scan's end)."""
    from torchdet3d.dataloaders.jpeg import plan_roi
    names = [n for n, _ in C.matrix()]
    n = 0
    for h, w in C.SIZES:
        for sampling in C.SAMPLINGS:
            s = SAMPLING[sampling]
            info, segs = _index(names.index(f'{h}x{w}_{sampling}_q90_0'), seg_mcus)
            X, S, nseg, scan = int(info['mcus_x']), int(info['seg_mcus']), int(info['nseg']), int(info['scan_bytes'])
            byte = [int(b) for b in segs['byte']] + [scan]
            dw = (w + 1) >> 1
            if small(h, w):
                ys = list(_Axis(h, s, dw).spans())
                rects = ((x0, y0, x1, y1, mx0, my0, mx1, my1) for x0, x1, mx0, mx1 in _Axis(w, s, dw).spans() for y0, y1, my0, my1 in ys)
            else:
                rects = []
                for r in _rects(h, w, h * w + seg_mcus % 7):
                    m = marked(s, h, w, *r)
                    rects.append(r + (min(b for _, b in m), min(a for a, _ in m), max(b for _, b in m) + 1, max(a for a, _ in m) + 1))
            seen = {}
            for x0, y0, x1, y1, mx0, my0, mx1, my1 in rects:
                p = plan_roi(info, segs, x0, y0, x1, y1)
                assert p['rect'] == (x0, y0, x1, y1) and p['mcus'] == (mx0, my0, mx1, my1)
                assert p['runs'] == (y1 - y0) * -(-(x1 - x0) // 4)
                rest = (p['row_segs'].tolist(), p['seg_first'], p['seg_count'], p['span'], p['blocks'], p['lanes'])
                if p['mcus'] in seen:               # (what follows depends on the MCU rectangle alone: checked once for each)
                    assert rest == seen[p['mcus']]
                    n += 1
                    continue
                seen[p['mcus']] = rest
                want = sorted({(a * X + b) // S for a in range(my0, my1) for b in range(mx0, mx1)})      # the marked MCUs' owners
                got = [t for a, b in p['row_segs'] for t in range(int(a), int(b))]
                assert got == want, (h, w, sampling, x0, y0, x1, y1)
                assert len(p['row_segs']) == my1 - my0
                for r, (a, b) in enumerate(p['row_segs']):      # a row's segments own an MCU of that row
                    assert all((my0 + r) * X + mx0 < (t + 1) * S and t * S <= (my0 + r) * X + mx1 - 1 for t in range(int(a), int(b)))
                assert p['seg_first'] == want[0] and p['seg_first'] + p['seg_count'] == want[-1] + 1
                first, nbytes = p['span']
                assert 0 <= first and nbytes >= 1 and first + nbytes <= scan
                for t in want:
                    assert first <= byte[t] and min(byte[t + 1] + 1, scan) <= first + nbytes
                assert p['blocks'] == (mx1 - mx0) * (my1 - my0) * (1, 3, 6)[s]
                assert p['lanes'] >= len(want)
                n += 1
            assert nseg == len(segs)
    assert n > 110000
