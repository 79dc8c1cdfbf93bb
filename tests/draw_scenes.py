"""The scenes of the draw tests (tests/test_draw_host.py asserts on the reference's owner map that they contain what they
claim; tests/test_gpu_draw.py holds the kernel to the reference on them)."""
import functools

import numpy as np

T = 5
IDS = (3, 7, -1, 12, 0)
LABELS = (0, 3, 6, 8, 20)          # bike, cereal_box, cup, shoe, and a label without a class name


def cube(cx, cy, a, d):
    """Keypoints of a box drawn in cabinet projection: the centre, then the vertices 1..8 with the corner signs of
    csrc/box_geometry.h (x the slowest bit, z the fastest)."""
    pts = [(cx, cy)]
    for i in range(8):
        sx, sy, sz = (i >> 2) & 1, (i >> 1) & 1, i & 1
        pts.append((cx + (a if sx else -a) + (d if sz else 0), cy + (a if sy else -a) - (d // 2 if sz else 0)))
    return np.array(pts, np.float64).reshape(18)


@functools.lru_cache(maxsize=None)
def scene(S, H, W, seed=0):
    """Noise frames and five objects per camera (cameras differ in `count` only: the last has 5, the one before 1, the one
    before that 0 -- rows past the count hold real objects that must not be drawn):
      0  a box with half-integer keypoints (round half even), id 3, 'bike';
      1  overlaps object 0; its plate ('cereal_box 7') runs over the right border;
      2  id -1: grey rectangle, no edges, no discs, plate clamped at the top row;
      3  over the left and top borders, keypoint 4 NaN and keypoint 0 inf (skipped with their edges);
      4  over the right and bottom borders, keypoints at +-9000 (invalid) and far above the frame (valid: its edges
         leave through the top row), a label without a name."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8)
    kp = np.zeros((S, T, 18))
    boxes = np.zeros((S, T, 4), np.int32)
    kp[:, 0], boxes[:, 0] = cube(14.5, 21.5, 5, 4), (5, 12, 30, 30)
    kp[:, 1], boxes[:, 1] = cube(33, 26, 6, 5), (20, 18, 50, 34)
    kp[:, 2], boxes[:, 2] = cube(50, 7, 3, 2), (40, 2, 60, 12)
    kp[:, 3], boxes[:, 3] = cube(3, 9, 5, 3), (-6, -4, 12, 16)
    kp[:, 3, 8], kp[:, 3, 0] = np.nan, np.inf
    kp[:, 4], boxes[:, 4] = cube(W - 4, H - 4, 6, 4), (W - 12, H - 10, W + 5, H + 6)
    kp[:, 4, 16:18], kp[:, 4, 14:16], kp[:, 4, 12] = (9000.0, 10.0), (W - 30.0, -3000.0), -9000.0
    ids = np.tile(np.array(IDS, np.int32), (S, 1))
    labels = np.tile(np.array(LABELS, np.int32), (S, 1))
    count = np.array([0, 1, 5][-S:] if S <= 3 else [5] * S, np.int32)
    for a in (frames, kp, boxes, ids, labels, count):
        a.setflags(write=False)
    return dict(frames=frames, kp=kp, boxes=boxes, ids=ids, labels=labels, count=count)


@functools.lru_cache(maxsize=None)
def many(seed=1):
    """T = 1024 tiny objects on one 64 x 128 frame: every bit of the kernel's primitive mask is in use."""
    rng = np.random.default_rng(seed)
    H, W, n = 64, 128, 1024
    frames = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    cx, cy = rng.integers(-2, W + 2, n), rng.integers(-2, H + 2, n)
    kp = np.stack([cube(int(x), int(y), 1, 1) for x, y in zip(cx, cy)]).reshape(1, n, 18)
    boxes = np.stack([cx - 2, cy - 2, cx + 2, cy + 2], 1).astype(np.int32).reshape(1, n, 4)
    ids = rng.integers(-1, 3000, (1, n)).astype(np.int32)
    labels = np.where(rng.random((1, n)) < 0.03, rng.integers(0, 9, (1, n)), -1).astype(np.int32)
    count = np.array([n], np.int32)
    for a in (frames, kp, boxes, ids, labels, count):
        a.setflags(write=False)
    return dict(frames=frames, kp=kp, boxes=boxes, ids=ids, labels=labels, count=count)
