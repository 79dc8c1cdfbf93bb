"""The Objectron evaluation protocol as plain per-frame / per-box / per-threshold Python loops in fp64
numpy -- the restatement the device stage (csrc/objectron_eval.hip, torchdet3d/evaluation/objectron_eval.py) is held to --
and a scene generator.  A helper, not a test module.  The lift and the box-box IoU are the oracle's (oracle/geometry.py,
oracle/box_iou.py); everything else follows the reference's scripts/objectron_eval.py:116-175 and the published evaluator
(parity with the absent objectron package is unpinned)."""
import numpy as np

from oracle import geometry as OG
from oracle.box_iou import UNIT, Box, IoU

VIS, MAX_PIXEL, MAX_AZIMUTH, MAX_POLAR, MAX_DIST, NBINS = 0.1, 0.1, 30.0, 20.0, 1.0, 21
METRICS = ('pixel', 'azimuth', 'polar', 'iou', 'add', 'adds')
HI = dict(pixel=MAX_PIXEL, azimuth=MAX_AZIMUTH, polar=MAX_POLAR, iou=1.0, add=MAX_DIST, adds=MAX_DIST)
THRESHOLDS = {m: np.linspace(0.0, HI[m], NBINS) for m in METRICS}


# ---- steps 1-4 -------------------------------------------------------------------------------------------------------------------
def num_instances(kp2d, kp3d, vis):
    n = 0
    for inst, inst3, v in zip(kp2d, kp3d, vis):
        if v > VIS and 0 < inst[0][0] < 1 and 0 < inst[0][1] < 1 and inst3[0, 2] < 0:
            n += 1
    return n


def match_box(pred, kp2d, vis):
    if len(kp2d) == 0:
        return -1
    i = int(np.argmin([np.linalg.norm(pred[1:] - inst[1:]) for inst in kp2d]))
    return -1 if vis[i] < VIS else i


def compute_scale(box, plane):
    center, normal = plane
    d = np.sort([np.dot(v, normal) for v in box[1:]])
    with np.errstate(all='ignore'):
        return np.mean(np.dot(center, normal) / d[:4])


def viewpoint(v):
    size = np.array([np.linalg.norm(v[5] - v[1]), np.linalg.norm(v[3] - v[1]), np.linalg.norm(v[2] - v[1])])
    oh = np.concatenate([UNIT * size, np.ones((9, 1))], 1).T
    vh = np.concatenate([v, np.ones((9, 1))], 1).T
    try:
        t = oh @ vh.T @ np.linalg.inv(vh @ vh.T)
    except np.linalg.LinAlgError:
        return np.nan, np.nan
    x, y, z = t[0, 3], t[1, 3], t[2, 3]
    return np.degrees(np.arctan2(z, x)), np.degrees(np.arctan2(y, np.hypot(x, z)))


def box_iou(a, b):
    try:
        r = IoU(Box(a), Box(b)).iou()
    except Exception:      # noqa: BLE001  (LinAlgError / QhullError / non-finite vertices: the project's IoU gives 0)
        return 0.0
    return float(r) if np.isfinite(r) else 0.0


def evaluate_box(pred, kp2d, kp3d, vis, plane):
    """-> (pixel, azimuth, polar, iou, add, adds), matched index."""
    i = match_box(pred, kp2d, vis)
    if i < 0:
        return (MAX_PIXEL, MAX_AZIMUTH, MAX_POLAR, 0.0, MAX_DIST, MAX_DIST), -1
    pixel = np.mean([np.linalg.norm(pred[k] - kp2d[i][k]) for k in range(1, 9)])
    box = OG.lift_2d([pred], portrait=True)[0]
    box = box * compute_scale(box, plane)
    az_p, po_p = viewpoint(box)
    az_g, po_g = viewpoint(kp3d[i])
    polar = abs(po_p - po_g)
    az = abs(az_p - az_g)
    if az > 180:
        az = 360 - az
    add = np.mean([np.linalg.norm(box[k] - kp3d[i][k]) for k in range(9)])
    adds = np.mean([np.min([np.linalg.norm(box[k] - kp3d[i][j]) for j in range(9)]) for k in range(9)])
    return (float(pixel), float(az), float(polar), box_iou(box, kp3d[i]), float(add), float(adds)), i


# ---- step 5 ----------------------------------------------------------------------------------------------------------------------
def evaluate_frames(frames):
    """frames: dicts with pred [P_f,9,2], kp2d [G_f,9,2], kp3d [G_f,9,3], vis [G_f], plane (centre, normal).  One entry per
    frame: metrics [P_f,6], matched [P_f], valid, n (= G_f), hit / miss [6,21], sums [5]."""
    out = []
    for fr in frames:
        res = [evaluate_box(p, fr['kp2d'], fr['kp3d'], fr['vis'], fr['plane']) for p in fr['pred']]
        metrics = np.array([r[0] for r in res], np.float64).reshape(-1, 6)
        matched = np.array([r[1] for r in res], np.int32)
        valid = num_instances(fr['kp2d'], fr['kp3d'], fr['vis']) > 0
        hit, miss, sums = np.zeros((6, NBINS), np.int32), np.zeros((6, NBINS), np.int32), np.zeros(5)
        if valid:
            for vals, mi in zip(metrics, matched):
                for m, name in enumerate(METRICS):
                    for j, t in enumerate(THRESHOLDS[name]):
                        h = vals[m] >= t if name == 'iou' else vals[m] <= t
                        hit[m, j] += bool(h)
                        miss[m, j] += not h
                if mi >= 0:
                    for s, m in enumerate((0, 3, 1, 2)):          # error_2d, iou_3d, azimuth, polar
                        if np.isfinite(vals[m]):
                            sums[s] += vals[m]
                    sums[4] += 1
        out.append(dict(metrics=metrics, matched=matched, valid=valid, n=len(fr['kp2d']), hit=hit, miss=miss, sums=sums))
    return out


# ---- step 6 ----------------------------------------------------------------------------------------------------------------------
def average_precision(hit, miss, total):
    """hit / miss: per-frame counts of one (metric, threshold) in evaluation order."""
    tp, fp = 0.0, 0.0
    recall, precision = [0.0], [0.0]
    for h, m in zip(hit, miss):
        tp += h
        fp += m
        recall.append(tp / total)
        precision.append(tp / (tp + fp) if tp + fp > 0 else 0.0)
    recall.append(1.0)
    precision.append(0.0)
    for i in range(len(precision) - 2, -1, -1):
        precision[i] = max(precision[i], precision[i + 1])
    ap = 0.0
    for i in range(1, len(recall)):
        if recall[i] != recall[i - 1]:
            ap += (recall[i] - recall[i - 1]) * precision[i]
    return ap


def finalize(rows):
    rows = [r for r in rows if r['valid']]
    total = sum(r['n'] for r in rows)
    sums = np.sum([r['sums'] for r in rows], 0) if rows else np.zeros(5)
    matched = int(sums[4])
    aps = {name: np.array([average_precision([r['hit'][m, j] for r in rows], [r['miss'][m, j] for r in rows], total) if total else 0.0
                           for j in range(NBINS)]) for m, name in enumerate(METRICS)}
    mean = lambda v: v / matched if matched else 0.0      # noqa: E731
    return dict(aps=aps, thresholds=THRESHOLDS, error_2d=mean(sums[0]), iou_3d=mean(sums[1]), azimuth=mean(sums[2]),
                polar=mean(sums[3]), matched=matched, total_instances=total, frames=len(rows))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
NDC_CAM = OG.camera_matrix_to_ndc(OG.default_camera_matrix())


def project(points):
    """Camera-frame points [n,3] (z < 0) -> keypoints normalised to the frame, in the portrait convention lift_2d(portrait=True)
    inverts: ndc_x = kp_y * 2 - 1, ndc_y = kp_x * 2 - 1."""
    uv = OG.project_3d_points(points, NDC_CAM)
    return np.stack([(uv[:, 1] + 1) / 2, (uv[:, 0] + 1) / 2], 1)


def random_instance(rng, visibility=1.0):
    """A cuboid (R, t, s) in front of the camera: kp2d, kp3d, visibility and its plane (bottom-face centre, up axis)."""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    z = -rng.uniform(1.5, 3.0)
    t = np.array([rng.uniform(-0.25, 0.25) * z, rng.uniform(-0.25, 0.25) * z, z])
    s = rng.uniform(0.2, 0.5, 3)
    kp3d = (UNIT * s) @ q.T + t
    plane = (t - q[:, 1] * s[1] / 2, q[:, 1].copy())
    return dict(kp2d=project(kp3d), kp3d=kp3d, vis=visibility, plane=plane)


def make_frame(instances, preds, plane=None):
    """instances: random_instance dicts; preds: [n,9,2]; the plane is the first instance's unless given."""
    return dict(pred=np.asarray(preds, np.float64).reshape(-1, 9, 2), kp2d=np.array([i['kp2d'] for i in instances]).reshape(-1, 9, 2),
                kp3d=np.array([i['kp3d'] for i in instances]).reshape(-1, 9, 3), vis=np.array([i['vis'] for i in instances], np.float64),
                plane=plane if plane is not None else instances[0]['plane'])


def pack(frames, P, G, fill=0.0):
    """Padded arrays for the device: pred [F,P,9,2], pred_count [F], kp2d [F,G,9,2], kp3d [F,G,9,3], vis [F,G], gt_count [F],
    planes [F,6]; rows past the counts hold `fill`."""
    F = len(frames)
    a = dict(pred=np.full((F, P, 9, 2), fill), pred_count=np.zeros(F, np.int32), kp2d=np.full((F, G, 9, 2), fill),
             kp3d=np.full((F, G, 9, 3), fill), vis=np.full((F, G), fill), gt_count=np.zeros(F, np.int32), planes=np.zeros((F, 6)))
    for f, fr in enumerate(frames):
        n, g = len(fr['pred']), len(fr['kp2d'])
        a['pred'][f, :n], a['pred_count'][f] = fr['pred'], n
        a['kp2d'][f, :g], a['kp3d'][f, :g], a['vis'][f, :g], a['gt_count'][f] = fr['kp2d'], fr['kp3d'], fr['vis'], g
        a['planes'][f, :3], a['planes'][f, 3:] = fr['plane']
    return a


def six_frame_scene(seed):
    """The GPU test's scene (P = G = 3): 1. one object, exact prediction; 2. two objects, three noisy predictions, two on the
    same instance; 3. no prediction; 4. every instance invisible or behind the camera (an invalid frame); 5. a prediction
    nearest to an instance with visibility < VIS, and one on a visible instance; 6. three objects, three predictions."""
    rng = np.random.default_rng(seed)
    noisy = lambda inst, s: inst['kp2d'] + rng.normal(0, s, (9, 2))       # noqa: E731
    a = random_instance(rng)
    f1 = make_frame([a], [a['kp2d']])
    b, c = random_instance(rng), random_instance(rng)
    f2 = make_frame([b, c], [noisy(b, 0.004), noisy(c, 0.006), noisy(b, 0.008)])
    f3 = make_frame([random_instance(rng)], [])
    d, e = random_instance(rng, visibility=0.05), random_instance(rng)
    e['kp3d'] = e['kp3d'] * np.array([1.0, 1.0, -1.0])                   # z > 0
    f4 = make_frame([d, e], [noisy(d, 0.005)])
    g, h = random_instance(rng, visibility=0.05), random_instance(rng)
    f5 = make_frame([g, h], [noisy(g, 0.004), noisy(h, 0.005)], plane=h['plane'])
    i, j, k = random_instance(rng), random_instance(rng), random_instance(rng)
    f6 = make_frame([i, j, k], [noisy(k, 0.003), noisy(i, 0.007), noisy(j, 0.005)], plane=j['plane'])
    return [f1, f2, f3, f4, f5, f6]
