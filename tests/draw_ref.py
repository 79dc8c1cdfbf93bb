"""The raster rules of the draw stage (include/t3d.h: t3d_draw_overlays_u8) restated in numpy int64.

Painter's order, written as plain overdraw: objects in index order, within an object rectangle, 12 edges, 9 discs, plate,
text; a later primitive overwrites an earlier one.  The kernel walks the same order backwards and stops at the first hit, so
the two must agree bit for bit.  The font comes in as an argument (`t3d_draw_glyphs` copies it out of the library): there is
no second copy of the glyph table in Python.

`draw_ref` returns the image and, per pixel, the slot 24 * t + k of the primitive that owns it (-1: none): k = 0 rectangle,
1..12 edges, 13..21 discs, 22 plate, 23 text.  `full=True` tests every primitive against every pixel of the frame; the default
tests it inside its bounding box only (tests/test_draw_host.py holds the two forms to each other)."""
import numpy as np

CLASSES = ('bike', 'book', 'bottle', 'cereal_box', 'camera', 'chair', 'cup', 'laptop', 'shoe')
# csrc/box_geometry.h: c_edges (vertex numbers = keypoint indices 1..8): four along x, four along y, four along z
EDGES = ((1, 5), (2, 6), (3, 7), (4, 8), (1, 3), (5, 7), (2, 4), (6, 8), (1, 2), (3, 4), (5, 6), (7, 8))
SLOTS = 24
K_RECT, K_EDGE0, K_DISC0, K_PLATE, K_TEXT = 0, 1, 13, 22, 23
LIM = 8191
C_RECT, C_RECT_OFF, C_EDGE_X, C_EDGE_Y, C_EDGE_Z, C_KP, C_PLATE, C_TEXT = range(8)
DRAW_IDS = 1
GLYPH_CHARS = 'abcdefghijklmnopqrstuvwxyz0123456789_ '


def point(kp, i):
    """P_i = rint of (x, y), half to even; None unless both are finite and |.| <= 8191."""
    v = np.rint(np.asarray(kp, np.float64).reshape(-1)[2 * i:2 * i + 2])
    if not np.all(np.isfinite(v)) or np.any(np.abs(v) > LIM):
        return None
    return int(v[0]), int(v[1])


def seg_covers(xs, ys, a, b, th):
    abx, aby = b[0] - a[0], b[1] - a[1]
    apx, apy = xs - a[0], ys - a[1]
    L2 = abx * abx + aby * aby
    cap_a = 4 * (apx * apx + apy * apy) <= th * th
    if L2 == 0:
        return cap_a
    dot = apx * abx + apy * aby
    bpx, bpy = xs - b[0], ys - b[1]
    cap_b = 4 * (bpx * bpx + bpy * bpy) <= th * th
    cross = apx * aby - apy * abx
    body = 4 * cross * cross <= th * th * L2
    return np.where(dot <= 0, cap_a, np.where(dot >= L2, cap_b, body))


def disc_covers(xs, ys, c, r):
    dx, dy = xs - c[0], ys - c[1]
    return dx * dx + dy * dy <= r * r


def outline_covers(xs, ys, box, th):
    x0, y0, x1, y1 = box
    h0, h1 = th // 2, (th - 1) // 2
    outer = (xs >= x0 - h0) & (xs <= x1 + h1) & (ys >= y0 - h0) & (ys <= y1 + h1)
    inner = (xs >= x0 + h1 + 1) & (xs <= x1 - h0 - 1) & (ys >= y0 + h1 + 1) & (ys <= y1 - h0 - 1)
    return outer & ~inner


def fill_covers(xs, ys, box):
    return (xs >= box[0]) & (xs <= box[2]) & (ys >= box[1]) & (ys <= box[3])


def glyph_index(ch):
    i = GLYPH_CHARS.find(ch)
    return i if i >= 0 else len(GLYPH_CHARS)          # any other character: the filled cell


def text_covers(xs, ys, origin, k, text, glyphs):
    n = len(text)
    if isinstance(glyphs, (bytes, bytearray)):
        glyphs = np.frombuffer(glyphs, np.uint8)
    table = np.vstack([np.asarray(glyphs, np.int64).reshape(len(GLYPH_CHARS), 7), np.full((1, 7), 0x1f, np.int64)])
    gi = np.array([glyph_index(c) for c in text], np.int64)
    dx, dy = xs - origin[0], ys - origin[1]
    cx, cy = dx // k, dy // k                          # floor division: negative offsets stay negative
    ok = (cx >= 0) & (cx < 6 * n) & (cy >= 0) & (cy < 7) & (cx % 6 < 5)
    ci, cyc, col = np.clip(cx // 6, 0, n - 1), np.clip(cy, 0, 6), np.clip(cx % 6, 0, 4)
    return ok & (((table[gi[ci], cyc] >> (4 - col)) & 1) == 1)


def label_text(label, ident, flags):
    text = CLASSES[label] if 0 <= label < len(CLASSES) else ''
    if (flags & DRAW_IDS) and ident >= 0:
        text += ' ' + str(int(ident))
    return text


def primitives(kp, box, ident, has_ids, label, style):
    """The up to 24 primitives of one object: [(k, colour index, closed bounding box, coverage function)], in layer order."""
    out = []
    th_r, th_e, rad, ks, flags = style.rect_th, style.edge_th, style.kp_radius, style.font_scale, style.flags
    off = has_ids and ident < 0
    if box is not None:
        b = [int(min(max(int(v), -LIM - 1), LIM)) for v in box]
        box = (min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3]))
        h0, h1 = th_r // 2, (th_r - 1) // 2
        out.append((K_RECT, C_RECT_OFF if off else C_RECT, (box[0] - h0, box[1] - h0, box[2] + h1, box[3] + h1),
                    lambda xs, ys, box=box: outline_covers(xs, ys, box, th_r)))
    if not off:
        pts = [point(kp, i) for i in range(9)]
        m = (th_e + 1) // 2
        for e, (i, j) in enumerate(EDGES):
            a, b = pts[i], pts[j]
            if a is None or b is None:
                continue
            bb = (min(a[0], b[0]) - m, min(a[1], b[1]) - m, max(a[0], b[0]) + m, max(a[1], b[1]) + m)
            out.append((K_EDGE0 + e, C_EDGE_X + e // 4, bb, lambda xs, ys, a=a, b=b: seg_covers(xs, ys, a, b, th_e)))
        for i, c in enumerate(pts):
            if c is None:
                continue
            out.append((K_DISC0 + i, C_KP, (c[0] - rad, c[1] - rad, c[0] + rad, c[1] + rad),
                        lambda xs, ys, c=c: disc_covers(xs, ys, c, rad)))
    text = label_text(label, ident if has_ids else -1, flags)
    n = len(text)
    if n:
        px, py = (box[0], max(box[1] - 9 * ks, 0)) if box is not None else (0, 0)
        plate = (px, py, px + (6 * n - 1) * ks + 2 * ks - 1, py + 9 * ks - 1)
        out.append((K_PLATE, C_PLATE, plate, lambda xs, ys: fill_covers(xs, ys, plate)))
        org = (px + ks, py + ks)
        out.append((K_TEXT, C_TEXT, (org[0], org[1], org[0] + 6 * n * ks - 1, org[1] + 7 * ks - 1),
                    lambda xs, ys: text_covers(xs, ys, org, ks, text, style.glyphs)))
    return out


class Style:
    """What the rules read of a style: the fields of t3d_draw_style (anything with those attributes, e.g. the packed ctypes
    struct of torchdet3d.utils.DrawStyle) plus the glyph table."""

    def __init__(self, packed, glyphs):
        self.rect_th, self.edge_th, self.kp_radius = int(packed.rect_th), int(packed.edge_th), int(packed.kp_radius)
        self.font_scale, self.flags = int(packed.font_scale), int(packed.flags)
        self.colors = np.array([[int(c) for c in row] for row in packed.colors], np.uint8).reshape(8, 3)
        self.glyphs = np.frombuffer(bytes(glyphs), np.uint8).reshape(len(GLYPH_CHARS), 7)


def draw_ref(frames, kp, glyphs, style, boxes=None, ids=None, labels=None, count=None, label_count=None, full=False):
    """frames uint8 [S,H,W,3], kp [S,T,18] float64, boxes [S,T,4] / ids [S,T] / labels [S,stride] / count [S] /
    label_count [S] integer arrays or None -> (image, owner int32 [S,H,W])."""
    img = np.array(frames, np.uint8, copy=True)
    S, H, W, _ = img.shape
    kp = np.asarray(kp, np.float64).reshape(S, -1, 18)
    T = kp.shape[1]
    st = style if isinstance(style, Style) else Style(style, glyphs)
    own = np.full((S, H, W), -1, np.int32)
    for s in range(S):
        n = T if count is None else min(max(int(count[s]), 0), T)
        stride = 0 if labels is None else np.asarray(labels).shape[1]
        lc = stride if label_count is None else min(max(int(label_count[s]), 0), stride)
        for t in range(n):
            label = int(labels[s][t]) if labels is not None and t < lc else -1
            prims = primitives(kp[s, t], None if boxes is None else boxes[s][t], int(ids[s][t]) if ids is not None else -1,
                               ids is not None, label, st)
            for k, ci, bb, covers in prims:
                lx, ly, hx, hy = (0, 0, W - 1, H - 1) if full else (max(bb[0], 0), max(bb[1], 0), min(bb[2], W - 1), min(bb[3], H - 1))
                if lx > hx or ly > hy:
                    continue
                ys, xs = np.mgrid[ly:hy + 1, lx:hx + 1].astype(np.int64)
                m = covers(xs, ys)
                img[s, ly:hy + 1, lx:hx + 1][m] = st.colors[ci]
                own[s, ly:hy + 1, lx:hx + 1][m] = SLOTS * t + k
    return img, own
