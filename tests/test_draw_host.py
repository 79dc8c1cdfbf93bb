"""CPU: the draw stage's boundary (entry points, style packing, the font), known answers of the numpy restatement of the
raster rules (tests/draw_ref.py) and the claims of the GPU test scenes (tests/draw_scenes.py), asserted on the owner map."""
import ctypes
import os
import re

import numpy as np
import pytest

import draw_ref as R
from conftest import PKG
from draw_scenes import T, cube, scene


def _glyphs():
    from torchdet3d import _native as N
    n = N.lib().t3d_draw_glyphs(None, 0)
    buf = (ctypes.c_ubyte * n)()
    assert N.lib().t3d_draw_glyphs(buf, n) == n
    return bytes(buf)


def _style(**kw):
    from torchdet3d.utils import DrawStyle
    return R.Style(DrawStyle(**kw).pack(), _glyphs())


def _grid(h, w):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    return xs, ys


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_the_draw_api_is_exported():
    """(The two entry points, their types and the stage's place in a recorded plan: tests/test_abi.py.)"""
    from torchdet3d import utils
    for name in ('DrawStyle', 'draw_overlays', 'draw_kp'):
        assert hasattr(utils, name)


def test_style_packs_to_the_headers_struct():
    """(`DrawStyleC` against the compiler's layout of t3d_draw_style, 44 bytes: tests/test_abi.py.)"""
    from torchdet3d import _native as N
    from torchdet3d.utils import DrawStyle
    st = DrawStyle().pack()
    assert type(st) is N.DrawStyleC
    assert (st.rect_th, st.edge_th, st.kp_radius, st.font_scale, st.flags) == (2, 2, 3, 2, 0)
    cols = [tuple(row) for row in st.colors]
    assert cols == [(0, 255, 0), (100, 100, 100), (255, 0, 0), (0, 255, 0), (0, 0, 255), cols[5], (255, 255, 255), (0, 0, 0)]
    bgr = DrawStyle(bgr=True, draw_ids=True).pack()
    assert [tuple(row) for row in bgr.colors] == [c[::-1] for c in cols] and bgr.flags == R.DRAW_IDS
    for bad in (dict(rect_th=0), dict(rect_th=17), dict(edge_th=0), dict(kp_radius=33), dict(kp_radius=-1), dict(font_scale=0),
                dict(font_scale=9), dict(rect=(0, 0, 256)), dict(text=(1, 2)), dict(edge_th=1.5)):
        with pytest.raises(ValueError):
            DrawStyle(**bad).pack()


def test_the_font_has_38_distinct_glyphs():
    g = np.frombuffer(_glyphs(), np.uint8).reshape(-1, 7)
    assert g.shape[0] == len(R.GLYPH_CHARS) == 38
    assert (g < 32).all(), 'five columns'
    for ch, rows in zip(R.GLYPH_CHARS, g):
        assert rows.any() == (ch != ' '), ch
    assert len({bytes(r) for r in g}) == 38
    assert R.glyph_index('a') == 0 and R.glyph_index('9') == 35 and R.glyph_index('_') == 36 and R.glyph_index('?') == 38


def test_the_edge_order_is_box_geometrys():
    src = open(os.path.join(PKG, 'csrc', 'box_geometry.h')).read()
    line = re.search(r'c_edges\[12\]\[2\]\s*=\s*\{(.*?)\};', src, re.S).group(1)
    pairs = re.findall(r'\{(\d+),\s*(\d+)\}', line)
    assert tuple((int(a), int(b)) for a, b in pairs) == R.EDGES
    from torchdet3d.utils import OBJECTRON_CLASSES
    assert tuple(OBJECTRON_CLASSES) == R.CLASSES


# ---- known answers of the rules ----------------------------------------------------------------------------------------------------
def test_a_horizontal_thick_segment_is_a_bar_with_its_caps():
    xs, ys = _grid(12, 16)
    m = R.seg_covers(xs, ys, (5, 5), (10, 5), 3)
    want = (xs >= 4) & (xs <= 11) & (ys >= 4) & (ys <= 6)       # 4 d^2 <= 9: one pixel around, corners at d^2 = 2 included
    assert np.array_equal(m, want)


def test_a_thin_diagonal_is_the_diagonal():
    xs, ys = _grid(12, 12)
    m = R.seg_covers(xs, ys, (2, 2), (8, 8), 1)
    assert np.array_equal(m, (xs == ys) & (xs >= 2) & (xs <= 8))
    assert np.array_equal(R.seg_covers(xs, ys, (8, 8), (2, 2), 1), m)


@pytest.mark.parametrize('th', [1, 2, 3, 5])
def test_an_outline_side_is_th_pixels_wide(th):
    xs, ys = _grid(30, 40)
    m = R.outline_covers(xs, ys, (10, 8, 30, 22), th)
    row, col = m[15], m[:, 20]
    h0, h1 = th // 2, (th - 1) // 2
    assert np.flatnonzero(row).tolist() == list(range(10 - h0, 10 + h1 + 1)) + list(range(30 - h0, 30 + h1 + 1))
    assert np.flatnonzero(col).tolist() == list(range(8 - h0, 8 + h1 + 1)) + list(range(22 - h0, 22 + h1 + 1))
    assert row.sum() == col.sum() == 2 * th
    assert m[8 - h0].sum() == 21 + th - 1, 'the top side runs over both corners'


def test_a_zero_length_segment_is_a_disc():
    xs, ys = _grid(14, 14)
    assert np.array_equal(R.seg_covers(xs, ys, (6, 7), (6, 7), 4), R.disc_covers(xs, ys, (6, 7), 2))
    d2 = (xs - 6) ** 2 + (ys - 7) ** 2
    assert np.array_equal(R.seg_covers(xs, ys, (6, 7), (6, 7), 5), 4 * d2 <= 25)
    assert R.disc_covers(xs, ys, (6, 7), 0).sum() == 1


def test_points_round_half_to_even_and_reject_what_is_not_a_pixel():
    assert R.point([0.5, 1.5] + [0] * 16, 0) == (0, 2)
    assert R.point([2.5, -0.5] + [0] * 16, 0) == (2, 0)
    assert R.point([8191.4, -8191.4] + [0] * 16, 0) == (8191, -8191)          # (-8191.5 rounds to -8192: invalid, below)
    for bad in ([np.nan, 0], [0, np.inf], [-np.inf, 0], [8191.6, 0], [0, -8191.5], [9000, 0]):
        assert R.point(bad + [0] * 16, 0) is None, bad


def test_text_is_the_glyphs_scaled_and_other_characters_fill_their_cell():
    g = _glyphs()
    table = np.frombuffer(g, np.uint8).reshape(38, 7)
    xs, ys = _grid(30, 60)
    for k in (1, 2, 3):
        m = R.text_covers(xs, ys, (3, 2), k, 'a_?', g)
        for i, ch in enumerate('a_'):
            rows = table[R.glyph_index(ch)]
            cell = np.array([[(rows[r] >> (4 - c)) & 1 for c in range(5)] for r in range(7)], bool)
            got = m[2:2 + 7 * k, 3 + 6 * k * i:3 + 6 * k * i + 5 * k]
            assert np.array_equal(got, np.kron(cell, np.ones((k, k), bool))), (k, ch)
        assert m[2:2 + 7 * k, 3 + 12 * k:3 + 17 * k].all(), 'an unknown character is a filled cell'
        assert m.sum() == (m[2:2 + 7 * k, 3:3 + 17 * k]).sum(), 'nothing outside the cells, nothing in the gaps'
        assert not m[:, 3 + 5 * k:3 + 6 * k].any()
    assert R.label_text(3, 41, R.DRAW_IDS) == 'cereal_box 41' and R.label_text(3, -1, R.DRAW_IDS) == 'cereal_box'
    assert R.label_text(20, 0, R.DRAW_IDS) == ' 0' and R.label_text(-1, 5, 0) == '' and R.label_text(8, 5, 0) == 'shoe'


# ---- the scenes contain what they claim ---------------------------------------------------------------------------------------
SHAPES = [(3, 37, 70), (2, 32, 64)]


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def drawn(request):
    S, H, W = request.param
    sc = scene(S, H, W)
    st = _style(font_scale=1, draw_ids=True)
    img, own = R.draw_ref(sc['frames'], sc['kp'], None, st, boxes=sc['boxes'], ids=sc['ids'], labels=sc['labels'], count=sc['count'])
    return sc, st, img, own


def test_bounding_boxes_lose_nothing(drawn):
    sc, st, img, own = drawn
    img2, own2 = R.draw_ref(sc['frames'], sc['kp'], None, st, boxes=sc['boxes'], ids=sc['ids'], labels=sc['labels'],
                            count=sc['count'], full=True)
    assert np.array_equal(img, img2) and np.array_equal(own, own2)


def test_scene_counts_and_untouched_pixels(drawn):
    sc, st, img, own = drawn
    S = own.shape[0]
    for s in range(S):
        n = int(sc['count'][s])
        objs = set((own[s][own[s] >= 0] // R.SLOTS).tolist())
        assert objs == set(range(n)), (s, objs)
    keep = own < 0
    assert keep.any() and np.array_equal(img[keep], sc['frames'][keep])
    assert (img[~keep] != sc['frames'][~keep]).any()
    for s in range(S):
        for slot in np.unique(own[s][own[s] >= 0]):
            k = int(slot) % R.SLOTS
            ci = {R.K_RECT: None, R.K_PLATE: R.C_PLATE, R.K_TEXT: R.C_TEXT}.get(k, R.C_KP if k >= R.K_DISC0 else R.C_EDGE_X + (k - 1) // 4)
            if ci is not None:
                assert (img[s][own[s] == slot] == st.colors[ci]).all(), (s, slot)


def test_scene_has_an_overlap_between_two_objects(drawn):
    sc, st, img, own = drawn
    s = own.shape[0] - 1
    _, first = R.draw_ref(sc['frames'][s:], sc['kp'][s:], None, st, boxes=sc['boxes'][s:], ids=sc['ids'][s:], labels=sc['labels'][s:],
                          count=np.array([1]))
    both = (first[0] >= 0) & (own[s] // R.SLOTS == 1)
    assert both.any(), 'a pixel object 0 covers and object 1 owns'


def test_scene_is_cut_by_all_four_borders(drawn):
    sc, st, img, own = drawn
    S, H, W = own.shape
    s = S - 1
    prims = {}
    for t in range(T):
        for k, ci, bb, _ in R.primitives(sc['kp'][s, t], sc['boxes'][s, t], int(sc['ids'][s, t]), True, int(sc['labels'][s, t]), st):
            prims[R.SLOTS * t + k] = bb
    sides = dict(left=(own[s][:, 0], lambda bb: bb[0] < 0), top=(own[s][0], lambda bb: bb[1] < 0),
                 right=(own[s][:, W - 1], lambda bb: bb[2] > W - 1), bottom=(own[s][H - 1], lambda bb: bb[3] > H - 1))
    for name, (line, beyond) in sides.items():
        assert any(beyond(prims[int(slot)]) for slot in np.unique(line[line >= 0])), name


def test_scene_skips_invalid_points_and_the_edges_that_use_them(drawn):
    sc, st, img, own = drawn
    s = own.shape[0] - 1
    have = set(np.unique(own[s][own[s] >= 0]).tolist())
    ks3 = {k for k, *_ in R.primitives(sc['kp'][s, 3], sc['boxes'][s, 3], 12, True, 8, st)}
    assert R.K_DISC0 + 4 not in ks3 and R.K_DISC0 + 0 not in ks3 and R.K_DISC0 + 1 in ks3
    for e, (i, j) in enumerate(R.EDGES):
        assert (R.K_EDGE0 + e in ks3) == (4 not in (i, j)), e
    assert R.SLOTS * 3 + R.K_DISC0 + 7 in have and R.SLOTS * 3 + R.K_DISC0 + 4 not in have
    ks4 = {k for k, *_ in R.primitives(sc['kp'][s, 4], sc['boxes'][s, 4], 0, True, 20, st)}
    assert R.K_DISC0 + 8 not in ks4 and R.K_DISC0 + 6 not in ks4 and R.K_DISC0 + 7 in ks4, '+-9000 is no pixel, (W - 30, -3000) is'
    assert R.K_EDGE0 + 2 in ks4, 'the edge 3-7 runs to the far point'


def test_scene_has_an_untracked_object_with_its_plate_at_the_top_row(drawn):
    sc, st, img, own = drawn
    s = own.shape[0] - 1
    assert sc['ids'][s, 2] < 0
    slots = set((np.unique(own[s][own[s] // R.SLOTS == 2]) % R.SLOTS).tolist())
    assert slots == {R.K_RECT, R.K_PLATE, R.K_TEXT}, 'no edges, no discs'
    assert (img[s][own[s] == R.SLOTS * 2 + R.K_RECT] == st.colors[R.C_RECT_OFF]).all()
    assert (img[s][own[s] == R.SLOTS * 0 + R.K_RECT] == st.colors[R.C_RECT]).all()
    plate = own[s] == R.SLOTS * 2 + R.K_PLATE
    assert sc['boxes'][s, 2, 1] - 9 * st.font_scale < 0 and plate[0].any() and not plate[9 * st.font_scale:].any()
    # 'cup' only: the id is not appended to an untracked object
    text = (own[s] // R.SLOTS == 2) & (own[s] % R.SLOTS >= R.K_PLATE)
    assert np.flatnonzero(text.any(0)).max() == sc['boxes'][s, 2, 0] + (6 * 3 + 1) * st.font_scale - 1


def test_cube_fixture_follows_the_corner_signs():
    k = cube(10, 10, 2, 0).reshape(9, 2)
    assert k[0].tolist() == [10, 10] and k[1].tolist() == [8, 8] and k[5].tolist() == [12, 8] and k[3].tolist() == [8, 12]


# ---- draw_kp's argument errors (raised before anything touches the device) -------------------------------------------------------
def test_draw_kp_argument_errors():
    from torchdet3d.utils import draw_kp
    img, kp = np.zeros((8, 8, 3), np.uint8), np.zeros((9, 2))
    with pytest.raises(ValueError, match='num_keypoints'):
        draw_kp(img, kp, num_keypoints=8)
    for bad in ('car', 9, -1, 1.5, True, ('bike',)):
        with pytest.raises(ValueError, match='label'):
            draw_kp(img, kp, label=bad)
    with pytest.raises(ValueError, match='uint8'):
        draw_kp(img.astype(np.float32), kp)
    with pytest.raises(ValueError):
        draw_kp(np.zeros((8, 8), np.uint8), kp)
    with pytest.raises(ValueError):
        draw_kp(np.zeros((8, 8, 4), np.uint8), kp)
    with pytest.raises(ValueError, match='keypoints'):
        draw_kp(img, np.zeros((8, 2)))
