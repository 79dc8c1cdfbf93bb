"""Test helper (not a test module): plain-numpy restatement of the demo's IOU tracker (reference:
torchdet3d/utils/tracking_tools.py:127-290 `IOUTracker`, :9-124 `Track`) as csrc/track.hip runs it -- per frame: active
tracks in list order, cost 0.5 (1 - GIoU) rounded to float32, a minimum-cost assignment, gating on cost and IoU,
`add_detection` (gap interpolation, box EMA, keypoint filter with the optional `align_kp` swap search), new tracks in
detection order with ids from a FIFO of released ids, `_clear_old_tracks` with a stable compaction, then the
`get_tracked_objects` selection.  Like the kernel it keeps only the LAST box / keypoints and the length of a track, works in
fp64 throughout (the reference computes a new track's first update and interpolated entries in float32: a few 2^-24 on O(1)
keypoints) and takes an optional `max_tracks` cap: a detection that would open a track in a full table is dropped and counted.

`solve_assignment` is the textbook shortest-augmenting-path algorithm with row / column potentials (no scipy at test
time).  Every `process` also reports the frame's MARGINS -- how far each branch decision was from flipping -- so that a
comparison can stop at a frame whose outcome float rounding could change."""
from collections import deque

import numpy as np

PARAM_NAMES = ('time_window', 'continue_time_thresh', 'track_clear_thresh', 'match_threshold', 'track_detection_iou_thresh',
               'interpolate_time_thresh', 'detection_filter_speed', 'keypoints_filter_speed', 'add_treshold',
               'no_updated_frames_treshold', 'align_kp')
DEFAULTS = dict(time_window=5, continue_time_thresh=2, track_clear_thresh=3000, match_threshold=0.4,
                track_detection_iou_thresh=0.5, interpolate_time_thresh=10, detection_filter_speed=0.7,
                keypoints_filter_speed=0.3, add_treshold=0.1, no_updated_frames_treshold=5, align_kp=False)


def area(b):
    return max(b[2] - b[0], 0) * max(b[3] - b[1], 0)


def iou(b1, b2):
    inter = area([max(b1[0], b2[0]), max(b1[1], b2[1]), min(b1[2], b2[2]), min(b1[3], b2[3])])
    u = area(b1) + area(b2) - inter
    return inter / u if u > 0 else 0


def giou(b1, b2):
    inter = area([max(b1[0], b2[0]), max(b1[1], b2[1]), min(b1[2], b2[2]), min(b1[3], b2[3])])
    enclosing = area([min(b1[0], b2[0]), min(b1[1], b2[1]), max(b1[2], b2[2]), max(b1[3], b2[3])])
    u = area(b1) + area(b2) - inter
    v = inter / u if u > 0 else 0
    return v - (enclosing - u) / enclosing if enclosing > 0 else -1


def solve_assignment(cost):
    """Minimum-cost assignment of a rectangular matrix: every row (if rows <= columns) or every column gets a partner.
    -> (rows, cols) of the matched pairs, sorted by row.  fp64 arithmetic on the given costs; the arg-min over columns
    takes the lowest index among equals."""
    cost = np.asarray(cost, dtype=np.float64)
    transposed = cost.shape[0] > cost.shape[1]
    a = cost.T if transposed else cost
    n, m = a.shape
    if n == 0:
        return np.zeros(0, int), np.zeros(0, int)
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    p, way = np.zeros(m + 1, int), np.zeros(m + 1, int)         # p[j]: row (1-based) matched to column j; column 0 is virtual
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(m + 1, np.inf), np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = a[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            masked = np.where(used[1:], np.inf, minv[1:])
            j1 = int(np.argmin(masked)) + 1
            delta = masked[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    pairs = sorted((j - 1, p[j] - 1) if transposed else (p[j] - 1, j - 1) for j in range(1, m + 1) if p[j])
    return np.array([r for r, _ in pairs], int), np.array([c for _, c in pairs], int)


def _second_best_gap(cost, rows, cols):
    """Total of the best assignment that differs from (rows, cols), minus the optimum's total (inf when there is no other)."""
    best = cost[rows, cols].astype(np.float64).sum()
    gap = np.inf
    if min(cost.shape) == max(cost.shape) == 1:
        return gap
    for r, c in zip(rows, cols):
        alt = cost.astype(np.float64).copy()
        alt[r, c] = 1e6                           # any other assignment leaves out at least one of the optimum's pairs
        ar, ac = solve_assignment(alt)
        gap = min(gap, alt[ar, ac].sum() - best)
    return gap


def _dist(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return np.sqrt(dx * dx + dy * dy)


def _mean_dist(a, b):
    """Mean distance of 9 keypoint pairs, summed in index order (the kernel's order; np.mean's pairwise order differs in
    the last bit, 1e-16 against margins of 1e-4)."""
    s = 0.0
    for k in range(9):
        s += _dist(a[k], b[k])
    return s / 9


class _Track:
    __slots__ = ('id', 'box', 'kp', 'end', 'length', 'no_updated_frames')


class RefTracker:
    def __init__(self, max_tracks=None, **params):
        unknown = set(params) - set(PARAM_NAMES)
        assert not unknown, unknown
        self.p = dict(DEFAULTS, **params)
        self.max_tracks = max_tracks
        self.tracks, self.free_ids = [], deque()
        self.time = self.last_global_id = self.dropped = self.cleared = 0
        self.margins = {}

    @property
    def num_tracks(self):
        return len(self.tracks)

    def _margin(self, name, value):
        self.margins[name] = min(self.margins.get(name, np.inf), abs(float(value)))

    def min_margin(self):
        return min(self.margins.values(), default=np.inf)

    # ---- Track.add_detection --------------------------------------------------------------------------------------
    def _add_detection(self, tr, box, kp):
        p = self.p
        skip = self.time - tr.end
        prev_box, prev_kp = tr.box, tr.kp
        filtered = skip == 1
        if 1 < skip <= p['continue_time_thresh']:
            t = skip - 1                                        # only the last interpolated entry is looked at afterwards
            prev_box = [int(b1 + (b2 - b1) / skip * t) for b1, b2 in zip(tr.box, box)]
            prev_kp = tr.kp + (kp - tr.kp) / skip * t
            tr.length += skip - 1
            filtered = True
        tr.length += 1
        tr.end = self.time
        if not filtered:
            tr.box, tr.kp = list(box), kp.copy()
            return
        s = p['detection_filter_speed']
        tr.box = [int((1 - s) * a + s * b) for a, b in zip(prev_box, box)]
        new, prev = kp.reshape(9, 2), prev_kp.reshape(9, 2)
        dist = _mean_dist(new, prev)
        considered = new
        if p['align_kp']:
            idx, done = list(range(9)), [False] * 9
            for i in range(9):
                if done[i]:
                    continue
                distance = _dist(new[i], prev[i])
                best = i
                for j in range(i + 1, 9):
                    d = _dist(new[i], prev[j])
                    self._margin('align', d - distance)
                    if d < distance:                            # (`distance` stays what it was: the last such j wins)
                        best = j
                if best != i and not done[best]:
                    idx[i], idx[best] = best, i
                    done[i] = done[best] = True
            swapped = new[idx]
            after = _mean_dist(swapped, prev)
            if idx != list(range(9)):
                self._margin('align', after - dist)
            if after < dist:
                considered, dist = swapped, after
        self._margin('add_treshold', dist - p['add_treshold'])
        fs = p['keypoints_filter_speed']
        if dist < p['add_treshold']:
            tr.no_updated_frames = 0
            out = (1 - fs) * prev + fs * considered
        elif tr.no_updated_frames > p['no_updated_frames_treshold']:
            out = considered
        else:
            out = prev
            tr.no_updated_frames += 1
        tr.kp = np.array(out, dtype=np.float64).reshape(18)

    # ---- IOUTracker.process ---------------------------------------------------------------------------------------
    def process(self, boxes, kps):
        """boxes [n,4] integers (left, top, right, bottom), kps [n,18]."""
        p = self.p
        boxes = [[int(v) for v in b[:4]] for b in boxes]
        kps = [np.asarray(k, dtype=np.float64).reshape(18) for k in kps]
        assert len(boxes) == len(kps)
        self.margins = {}
        active = [i for i, tr in enumerate(self.tracks) if tr.end >= self.time - p['continue_time_thresh']]
        cost = np.zeros((len(boxes), len(active)), dtype=np.float32)
        for j, idx in enumerate(active):
            for i, d in enumerate(boxes):
                cost[i, j] = 0.5 * (1 - giou(d, self.tracks[idx].box))
        assignment = [None] * len(boxes)
        if cost.size:
            rows, cols = solve_assignment(cost)
            self._margin('assignment', _second_best_gap(cost, rows, cols))
            for i, j in zip(rows, cols):
                self._margin('match_threshold', float(cost[i, j]) - p['match_threshold'])
                if cost[i, j] < p['match_threshold']:
                    v = iou(self.tracks[active[j]].box, boxes[i])
                    self._margin('iou', v - p['track_detection_iou_thresh'])
                    if v > p['track_detection_iou_thresh']:
                        assignment[i] = j
            for i, j in enumerate(assignment):
                if j is not None:
                    self._add_detection(self.tracks[active[j]], boxes[i], kps[i])
        for i, j in enumerate(assignment):
            if j is None:
                if self.max_tracks is not None and len(self.tracks) >= self.max_tracks:
                    self.dropped += 1
                    continue
                tr = _Track()
                if self.free_ids:
                    tr.id = self.free_ids.popleft()
                else:
                    tr.id = self.last_global_id
                    self.last_global_id += 1
                tr.box, tr.kp, tr.end, tr.length, tr.no_updated_frames = list(boxes[i]), kps[i].copy(), self.time, 1, 0
                self.tracks.append(tr)
        kept = []
        for tr in self.tracks:
            if tr.end < self.time - p['track_clear_thresh']:
                self.cleared += 1
                continue
            if tr.end < self.time - p['continue_time_thresh'] and tr.length < p['time_window']:
                self.free_ids.append(tr.id)
                continue
            kept.append(tr)
        self.tracks = kept
        self.time += 1

    def tracked(self):
        """-> boxes [k,4] int64, kps [k,18] float64, ids [k] (-1: not longer than time_window) of the tracks the last
        frame touched, in track-list order."""
        sel = [tr for tr in self.tracks if tr.end == self.time - 1]
        boxes = np.array([tr.box for tr in sel], dtype=np.int64).reshape(-1, 4)
        kps = np.array([tr.kp for tr in sel], dtype=np.float64).reshape(-1, 18)
        ids = np.array([tr.id if tr.length > self.p['time_window'] else -1 for tr in sel], dtype=np.int64)
        return boxes, kps, ids


# ---- golden file access (tests/golden/tracker.npz, written by tools/gen_tracker_golden.py) ---------------------------
def load_scenes(path):
    """-> list of dicts: name, params, frames = [(boxes [n,4] int32, kps [n,18] float32)], expected = [(boxes, kps, ids,
    num_tracks, last_global_id)] per frame."""
    z = np.load(path)
    scenes = []
    for k, name in enumerate(z['names']):
        g = lambda f: z[f'in{int(z[f"s{k}_seed"])}_{f}' if f.startswith('det_') else f's{k}_{f}']
        ints, floats = g('params_int'), g('params_float')
        params = dict(time_window=int(ints[0]), continue_time_thresh=int(ints[1]), track_clear_thresh=int(ints[2]),
                      interpolate_time_thresh=int(ints[3]), no_updated_frames_treshold=int(ints[4]), align_kp=bool(ints[5]),
                      match_threshold=float(floats[0]), track_detection_iou_thresh=float(floats[1]),
                      detection_filter_speed=float(floats[2]), keypoints_filter_speed=float(floats[3]),
                      add_treshold=float(floats[4]))
        di = np.concatenate([[0], np.cumsum(g('det_counts'))])
        oi = np.concatenate([[0], np.cumsum(g('out_counts'))])
        frames = [(g('det_boxes')[a:b], g('det_kps')[a:b]) for a, b in zip(di[:-1], di[1:])]
        expected = [(g('out_boxes')[a:b], g('out_kps')[a:b], g('out_ids')[a:b], int(nt), int(lg))
                    for a, b, nt, lg in zip(oi[:-1], oi[1:], g('num_tracks'), g('last_global_id'))]
        scenes.append(dict(name=str(name), params=params, frames=frames, expected=expected))
    return scenes


# ---- the synthetic scene recipe (shared by the golden generator and the randomised GPU test) ------------------------
def make_scene(seed, frames=48, blank_frame=None, zero_area_frames=(5, 17, 33)):
    """About six boxes drifting at up to 10 px/frame over a 1920x1080 canvas (90-320 px a side, +-5 px jitter), 20 % of the
    detections dropped per frame, one object alive in frames 8..29 and one born at frame 20, the order shuffled per frame,
    12 % of the keypoint vectors jumping (sigma 0.2, else 0.01), an isolated false positive every 11th frame, one zero-area
    detection on `zero_area_frames` and no detection at all on `blank_frame`.
    -> [(boxes [n,4] int32, kps [n,18] float32)] per frame."""
    rng = np.random.default_rng(seed)
    W, H = 1920, 1080
    objs = []
    for born, dies in [(0, frames)] * 6 + [(8, 30), (20, frames)]:
        size = rng.uniform(90, 320, 2)
        objs.append(dict(born=born, dies=dies, size=size, pos=rng.uniform(0, 1, 2) * (np.array([W, H]) - size),
                         vel=rng.uniform(-10, 10, 2), kp=rng.uniform(0.1, 0.9, 18)))
    out = []
    for t in range(frames):
        dets = []
        for o in objs:
            if not o['born'] <= t < o['dies']:
                continue
            o['pos'] = o['pos'] + o['vel']
            for a, lim in ((0, W), (1, H)):
                if o['pos'][a] < 0 or o['pos'][a] + o['size'][a] > lim:
                    o['vel'][a] = -o['vel'][a]
                    o['pos'][a] = min(max(o['pos'][a], 0), lim - o['size'][a])
            dropped, jump = rng.random() < 0.2, rng.random() < 0.12
            jit = rng.integers(-5, 6, 4)
            noise = rng.normal(0, 0.2 if jump else 0.01, 18)
            if dropped:
                continue
            box = np.concatenate([o['pos'], o['pos'] + o['size']]).astype(np.int64) + jit
            dets.append((box, (o['kp'] + noise).astype(np.float32)))
        if t % 11 == 10:
            for _ in range(50):                                  # isolated: touching nothing else on the frame
                size = rng.uniform(90, 320, 2)
                pos = rng.uniform(0, 1, 2) * (np.array([W, H]) - size)
                box = np.concatenate([pos, pos + size]).astype(np.int64)
                if all(iou(box, d[0]) == 0 for d in dets):
                    break
            dets.append((box, rng.uniform(0.1, 0.9, 18).astype(np.float32)))
        if t in zero_area_frames:
            x, y, h = rng.integers(100, 1800), rng.integers(100, 900), rng.integers(90, 320)
            dets.append((np.array([x, y, x, y + h]), rng.uniform(0.1, 0.9, 18).astype(np.float32)))
        if t == blank_frame:
            dets = []
        order = rng.permutation(len(dets))
        out.append((np.array([dets[i][0] for i in order], dtype=np.int32).reshape(-1, 4),
                    np.array([dets[i][1] for i in order], dtype=np.float32).reshape(-1, 18)))
    return out
