"""The COCO bbox evaluation protocol of DESIGN.md section 7 as plain Python loops: a literal restatement of the published
pycocotools `COCOeval.evaluateImg` / `accumulate` / `summarize` (iouType 'bbox', useCats 1, no crowd annotations) in the
form mmdet 2.x's `CocoDataset.evaluate(metric='bbox')` drives it.  Written independently of
torchdet3d/evaluation/detection_eval.py and sharing no code with it; fp64 python floats throughout, one operation at a time.
"""
import math

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


def cap_counts(out, cnt, max_per_img):
    """mmdet's max_per_img on one image: out [nc,K,6], cnt [nc] -> the survivors per class of the stable sort by score over
    the classes' valid rows concatenated."""
    nc, K = out.shape[:2]
    keys = []
    for c in range(nc):
        for i in range(min(max(int(cnt[c]), 0), K)):
            keys.append((float(out[c, i, 4]), c))
    order = np.argsort(-np.array([k[0] for k in keys], np.float32), kind='stable')[:max_per_img] if keys else []
    kept = [0] * nc
    for j in order:
        kept[keys[j][1]] += 1
    return np.array(kept, np.int32)


def scale_box(box, fx, fy):
    x1, y1, x2, y2 = (float(v) for v in box)
    X1, Y1, X2, Y2 = x1 * fx, y1 * fy, x2 * fx, y2 * fy
    return (X1, Y1, X2, Y2), (X2 - X1) * (Y2 - Y1)


def box_iou(d, ad, g, ag):
    iw = min(d[2], g[2]) - max(d[0], g[0])
    ih = min(d[3], g[3]) - max(d[1], g[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    i = iw * ih
    u = ad + ag - i
    return i / u


def evaluate_img(dets, gts, area_rng):
    """dets: [(box, area, score)] in score order, at most 100; gts: [(box, area)] in slot order.
    -> dtm [T][D], dtIg [T][D] (bools), number of non-ignored ground truths."""
    lo, hi = area_rng
    ignore = [(ag < lo or ag > hi) for _, ag in gts]
    # stable sort: the non-ignored first
    gtind = [i for i in range(len(gts)) if not ignore[i]] + [i for i in range(len(gts)) if ignore[i]]
    gt = [gts[i] for i in gtind]
    gt_ig = [ignore[i] for i in gtind]
    ious = [[box_iou(d[0], d[1], g[0], g[1]) for g in gt] for d in dets]
    T, D, G = len(IOU_THRS), len(dets), len(gt)
    gtm = [[False] * G for _ in range(T)]
    dtm = [[False] * D for _ in range(T)]
    dt_ig = [[False] * D for _ in range(T)]
    for tind, t in enumerate(IOU_THRS):
        for dind in range(D):
            iou = min([float(t), 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind][gind]:
                    continue
                if m > -1 and not gt_ig[m] and gt_ig[gind]:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind][dind] = gt_ig[m]
            dtm[tind][dind] = True
            gtm[tind][m] = True
    for dind, d in enumerate(dets):
        outside = d[1] < lo or d[1] > hi
        for tind in range(T):
            if not dtm[tind][dind] and outside:
                dt_ig[tind][dind] = True
    return dtm, dt_ig, sum(1 for v in gt_ig if not v)


def image_cells(out, cnt, gt_boxes, gt_labels, gt_count, ori_shape, in_w, in_h):
    """One image -> per class (dets, gts) scaled to the original frame.  out [nc,K,6], cnt [nc] (already capped)."""
    nc, K = out.shape[:2]
    h, w = int(ori_shape[0]), int(ori_shape[1])
    fx, fy = float(w) / float(in_w), float(h) / float(in_h)
    cells = []
    G = gt_boxes.shape[0]
    for c in range(nc):
        dets = []
        for i in range(min(min(max(int(cnt[c]), 0), K), 100)):
            box, area = scale_box(out[c, i, :4], fx, fy)
            dets.append((box, area, out[c, i, 4]))
        gts = []
        for g in range(min(max(int(gt_count), 0), G)):
            x1, y1, x2, y2 = (float(v) for v in gt_boxes[g])
            if not all(math.isfinite(v) for v in (x1, y1, x2, y2)) or not x2 > x1 or not y2 > y1 or int(gt_labels[g]) != c:
                continue
            gts.append(scale_box(gt_boxes[g], fx, fy))
        cells.append((dets, gts))
    return cells


def record_of(out, cnt, gt_boxes, gt_labels, gt_counts, ori_shapes, in_w, in_h, max_per_img):
    """A batch (numpy: out [B,nc,K,6] f32, cnt [B,nc], gt_boxes [B,G,4] f32, gt_labels [B,G], gt_counts [B], ori_shapes
    [B,2]) -> the record the device keeps: dict(score [B,nc,100] f32, dtm / dtig [B,nc,100] uint64 with bit a * 10 + t,
    ndt [B,nc], ngt [B,nc,4], valid [B]) and the capped counts."""
    B, nc = cnt.shape
    rec = dict(score=np.zeros((B, nc, 100), np.float32), dtm=np.zeros((B, nc, 100), np.uint64),
               dtig=np.zeros((B, nc, 100), np.uint64), ndt=np.zeros((B, nc), np.int32), ngt=np.zeros((B, nc, 4), np.int32),
               valid=np.ones(B, np.int32))
    capped = np.stack([cap_counts(out[b], cnt[b], max_per_img) for b in range(B)])
    for b in range(B):
        cells = image_cells(out[b], capped[b], gt_boxes[b], gt_labels[b], gt_counts[b], ori_shapes[b], in_w, in_h)
        for c, (dets, gts) in enumerate(cells):
            rec['ndt'][b, c] = len(dets)
            for d, det in enumerate(dets):
                rec['score'][b, c, d] = det[2]
            for a, rng in enumerate(AREA_RNG):
                dtm, dt_ig, npig = evaluate_img(dets, gts, rng)
                rec['ngt'][b, c, a] = npig
                for t in range(len(IOU_THRS)):
                    for d in range(len(dets)):
                        bit = np.uint64(1 << (a * 10 + t))
                        if dtm[t][d]:
                            rec['dtm'][b, c, d] |= bit
                        if dt_ig[t][d]:
                            rec['dtig'][b, c, d] |= bit
    return rec, capped


def accumulate(rec):
    """`COCOeval.accumulate` over a record (rows in evaluation order) -> precision [T,R,K,A,M], recall [T,K,A,M]."""
    n, nc = rec['ndt'].shape
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, nc, A, M))
    recall = -np.ones((T, nc, A, M))
    for k in range(nc):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                scores, cells, npig = [], [], 0
                for r in range(n):
                    if not rec['valid'][r]:
                        continue
                    nd = min(int(rec['ndt'][r, k]), max_det)
                    for d in range(nd):
                        scores.append(rec['score'][r, k, d])
                        cells.append((r, d))
                    npig += int(rec['ngt'][r, k, a])
                if npig == 0:
                    continue
                inds = np.argsort(-np.array(scores, np.float32), kind='mergesort') if scores else []
                for t in range(T):
                    bit = a * 10 + t
                    tp, fp, tps, fps = 0, 0, [], []
                    for j in inds:
                        r, d = cells[j]
                        hit = (int(rec['dtm'][r, k, d]) >> bit) & 1
                        ign = (int(rec['dtig'][r, k, d]) >> bit) & 1
                        tp += 1 if (hit and not ign) else 0
                        fp += 1 if (not hit and not ign) else 0
                        tps.append(float(tp))
                        fps.append(float(fp))
                    nd = len(tps)
                    rc = [v / npig for v in tps]
                    pr = [tps[i] / (fps[i] + tps[i] + np.spacing(1)) for i in range(nd)]
                    q = [0.0] * R
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    at = np.searchsorted(rc, REC_THRS, side='left')
                    try:
                        for ri, pi in enumerate(at):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def summarize(precision, recall):
    def _summarize(ap=1, iou_thr=None, area=0, max_dets=100):
        mind = MAX_DETS.index(max_dets)
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, area, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, area, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    stats = np.zeros(12)
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iou_thr=.5)
    stats[2] = _summarize(1, iou_thr=.75)
    stats[3] = _summarize(1, area=1)
    stats[4] = _summarize(1, area=2)
    stats[5] = _summarize(1, area=3)
    stats[6] = _summarize(0, max_dets=1)
    stats[7] = _summarize(0, max_dets=10)
    stats[8] = _summarize(0, max_dets=100)
    stats[9] = _summarize(0, area=1)
    stats[10] = _summarize(0, area=2)
    stats[11] = _summarize(0, area=3)
    return stats


def concat_records(recs):
    return {k: np.concatenate([r[k] for r in recs]) for k in recs[0]}
