"""numpy restatement of the SSD MultiBox loss (include/t3d.h: t3d_ssd_multibox_loss) -- with the header's text THE definition:
the published mmdet 2.x SSDHead.loss / MaxIoUAssigner(gt_max_assign_all=False) / DeltaXYWHBBoxCoder / smooth_l1_loss.

`multibox(...)` works on dense arrays (cls [B,A,nc+1], reg [B,A,4]); `dtype` is the precision of the per-anchor arithmetic
(float32 restates the kernel, float64 is the yardstick); the IoU is always float32 with every operation rounded on its own
(numpy rounds each array operation), so the assignment is the kernel's bit for bit; all sums are float64.
Also here: the inputs of every case the GPU tests run (`gpu_cases`), the float32-against-float64 spreads that bound the
kernel's error (`spreads`) and the mining-gap condition (`mining_gap`)."""
import functools
import math

import numpy as np

STDS = (0.1, 0.1, 0.2, 0.2)
NC = 9
F = np.float32


def iou_f32(g, anchors):
    """g [4], anchors [A,4] float32 -> [A] float32; one rounding per operation, as the kernel's __f*_rn chain."""
    g = np.asarray(g, F)
    a = np.asarray(anchors, F)
    iw = np.maximum(np.minimum(g[2], a[:, 2]) - np.maximum(g[0], a[:, 0]), F(0))
    ih = np.maximum(np.minimum(g[3], a[:, 3]) - np.maximum(g[1], a[:, 1]), F(0))
    inter = iw * ih
    area_g = (g[2] - g[0]) * (g[3] - g[1])
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    union = np.maximum((area_g + area_a) - inter, F(1e-6))
    return inter / union


def valid_slots(boxes, labels, count, nc):
    G = boxes.shape[0]
    count = min(max(int(count), 0), G)
    out = []
    for i in range(count):
        x1, y1, x2, y2 = (float(v) for v in boxes[i])
        if all(math.isfinite(v) for v in (x1, y1, x2, y2)) and x2 > x1 and y2 > y1 and 0 <= int(labels[i]) < nc:
            out.append(i)
    return out


def assign(anchors, boxes, labels, count, nc, pos_iou_thr=0.4, min_pos_iou=0.0):
    """-> assigned [A] int32 (ground-truth slot or -1)."""
    A = anchors.shape[0]
    best = np.full(A, -1.0, F)
    arg = np.full(A, -1, np.int32)
    slots = valid_slots(boxes, labels, count, nc)
    ious = {}
    for i in slots:
        v = ious[i] = iou_f32(boxes[i], anchors)
        up = v > best                   # strictly: the first ground truth keeps a tie
        best[up], arg[up] = v[up], i
    assigned = np.where(best >= F(pos_iou_thr), arg, -1).astype(np.int32)
    for i in slots:                     # ascending: a later ground truth overrides an earlier one
        v = ious[i]
        if v.max() >= F(min_pos_iou):
            assigned[int(np.argmax(v))] = i     # argmax: the lowest anchor attaining the maximum
    return assigned


def box_targets(anchors, g, stds, dtype):
    a, g = anchors.astype(dtype), np.asarray(g).astype(dtype)
    half = dtype(0.5)
    px, py, pw, ph = (a[:, 0] + a[:, 2]) * half, (a[:, 1] + a[:, 3]) * half, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    gx, gy, gw, gh = (g[:, 0] + g[:, 2]) * half, (g[:, 1] + g[:, 3]) * half, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    s = [dtype(F(v)) for v in stds]     # (the kernel holds the stds as float32)
    return np.stack([((gx - px) / pw) / s[0], ((gy - py) / ph) / s[1], np.log(gw / pw) / s[2], np.log(gh / ph) / s[3]], -1)


def softmax_ce(x, label, dtype):
    """x [A,C] -> (ce [A], softmax [A,C]); the class sum runs in channel order, as the kernel's."""
    x = x.astype(dtype)
    mx = x.max(-1)
    e = np.exp(x - mx[:, None])
    den = np.zeros(x.shape[0], dtype)
    for k in range(x.shape[1]):
        den = den + e[:, k]
    ce = np.log(den) - (x[np.arange(x.shape[0]), label] - mx)
    return ce, e / den[:, None]


def mine(ce, negative, k):
    """The k negatives first by (ce descending, anchor ascending); float32 ce is ordered on its bit pattern."""
    idx = np.nonzero(negative)[0]
    key = ce[idx].view(np.uint32).astype(np.int64) if ce.dtype == np.float32 else ce[idx]
    order = np.argsort(-key, kind='stable')
    return idx[order[:k]]


def multibox(cls, reg, anchors, gt_boxes, gt_labels, gt_counts, nc=NC, pos_iou_thr=0.4, neg_iou_thr=0.4, min_pos_iou=0.0,
             neg_pos_ratio=3, beta=1.0, stds=STDS, dtype=np.float32):
    assert pos_iou_thr == neg_iou_thr, 'no ignore band'
    dtype = np.dtype(dtype).type
    B, A = cls.shape[0], anchors.shape[0]
    anchors = np.asarray(anchors, F)
    assigned = np.full((B, A), -1, np.int32)
    num_pos = np.zeros(B, np.int32)
    ce_all = np.zeros((B, A), dtype)
    sm_all, lab_all = np.zeros((B, A, nc + 1), dtype), np.full((B, A), nc, np.int64)
    diff_all = np.zeros((B, A, 4), dtype)
    sum_cls, sum_box, mined_total, gaps = [], [], 0, []
    beta_t = dtype(F(beta))
    for b in range(B):
        asg = assign(anchors, gt_boxes[b], gt_labels[b], gt_counts[b], nc, pos_iou_thr, min_pos_iou) if gt_boxes.shape[1] else \
            np.full(A, -1, np.int32)
        pos = asg >= 0
        label = np.where(pos, gt_labels[b][np.maximum(asg, 0)] if gt_boxes.shape[1] else 0, nc).astype(np.int64)
        ce, sm = softmax_ce(cls[b], label, dtype)
        npos = int(pos.sum())
        k = min(neg_pos_ratio * npos, A - npos)
        mined = mine(ce, ~pos, k)
        gaps.append(mining_gap(ce, ~pos, k))
        asg = asg.copy()
        asg[mined] = -2
        used = asg != -1
        sum_cls.append(ce[used].astype(np.float64).sum())
        sb = 0.0
        if npos:
            t = box_targets(anchors[pos], gt_boxes[b][asg[pos]], stds, dtype)
            d = reg[b][pos].astype(dtype) - t
            ad = np.abs(d)
            l1 = np.where(ad < beta_t, dtype(0.5) * ad * ad / beta_t, ad - dtype(0.5) * beta_t)
            sb = l1.astype(np.float64).sum()
            diff_all[b][pos] = d
        sum_box.append(sb)
        assigned[b], num_pos[b], ce_all[b], sm_all[b], lab_all[b] = asg, npos, ce, sm, label
        mined_total += k
    total_pos = int(num_pos.sum())
    avg = max(total_pos, 1)
    avg_t = dtype(avg)
    onehot = np.zeros((B, A, nc + 1), dtype)
    np.put_along_axis(onehot, lab_all[..., None], dtype(1), -1)
    dcls = np.where((assigned != -1)[..., None], (sm_all - onehot) / avg_t, dtype(0))
    ad = np.abs(diff_all)
    g = np.where(ad < beta_t, diff_all / beta_t, np.sign(diff_all))
    dreg = np.where((assigned >= 0)[..., None], g / avg_t, dtype(0))
    return dict(loss_cls=float(np.sum(np.asarray(sum_cls, np.float64))) / avg, loss_bbox=float(np.sum(np.asarray(sum_box, np.float64))) / avg,
                total_pos=total_pos, total_mined=mined_total, num_pos=num_pos, assigned=assigned, dcls=dcls, dreg=dreg, ce=ce_all,
                labels=lab_all, gaps=gaps)


def mining_gap(ce, negative, k):
    """Relative distance between the ce at rank k and at rank k + 1 of the negatives (inf when the cut is not inside them)."""
    v = np.sort(ce[negative].astype(np.float64))[::-1]
    if k <= 0 or k >= v.size:
        return math.inf
    return float((v[k - 1] - v[k]) / max(abs(v[k - 1]), 1e-300))


def torch_loss(cls, reg, anchors, gt_boxes, ref):
    """The two losses as torch float64 functions of (cls, reg) for the restatement's assignment: what autograd differentiates."""
    import torch
    asg = torch.from_numpy(ref['assigned'].astype(np.int64))
    lab = torch.from_numpy(ref['labels'])
    used, pos = asg != -1, asg >= 0
    ce = torch.nn.functional.cross_entropy(cls.reshape(-1, cls.shape[-1]), lab.reshape(-1), reduction='none').view(asg.shape)
    avg = max(ref['total_pos'], 1)
    loss_cls = (ce * used).sum() / avg
    loss_bbox = cls.new_zeros(())
    for b in range(asg.shape[0]):
        if pos[b].any():
            idx = torch.nonzero(pos[b])[:, 0]
            t = torch.from_numpy(box_targets(anchors[idx.numpy()], gt_boxes[b][asg[b][idx].numpy()], STDS, np.float64))
            loss_bbox = loss_bbox + torch.nn.functional.smooth_l1_loss(reg[b][idx], t, reduction='sum', beta=1.0)
    return loss_cls, loss_bbox / avg


# ---- layouts: dense [B,A,C] <-> the head's per-level rows [B*hw][stride] with pad channels -------------------------------
def to_levels(dense, hws, nas, per_anchor, strides, pad=np.nan):
    B, out, o = dense.shape[0], [], 0
    for hw, na, st in zip(hws, nas, strides):
        lv = np.full((B * hw, st), pad, dense.dtype)
        lv[:, :na * per_anchor] = dense[:, o:o + hw * na].reshape(B * hw, na * per_anchor)
        out.append(lv)
        o += hw * na
    return out


def from_levels(levels, hws, nas, per_anchor, B):
    """-> (dense [B,A,per_anchor], the pad channels of all levels as one flat array)."""
    dense = [lv[:, :na * per_anchor].reshape(B, hw * na, per_anchor) for lv, hw, na in zip(levels, hws, nas)]
    pads = [lv[:, na * per_anchor:].ravel() for lv, na in zip(levels, nas)]
    return np.concatenate(dense, 1), np.concatenate(pads)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def small_anchors():
    """12 anchors: one level of 2 x 3 cells of 32 pixels (a 96 x 64 image), per cell the 32 x 32 cell itself and the 16 x 16
    box on its centre.  Index = (row * 3 + col) * 2 + anchor."""
    out = []
    for r in range(2):
        for c in range(3):
            cx, cy = 32 * c + 16, 32 * r + 16
            out += [[cx - 16, cy - 16, cx + 16, cy + 16], [cx - 8, cy - 8, cx + 8, cy + 8]]
    return np.asarray(out, F)


def real_anchors():
    from torchdet3d.models.ssd import make_anchors
    return make_anchors()


REAL_LEVELS = dict(hws=(19 * 19, 10 * 10), nas=(4, 6))
SMALL_LEVELS = dict(hws=(6,), nas=(2,))


def _logits(rng, B, A, bf16=False):
    cls = (rng.standard_normal((B, A, NC + 1)) * 2.0).astype(F)
    reg = rng.standard_normal((B, A, 4)).astype(F)
    if bf16:
        import torch
        cls = torch.from_numpy(cls).to(torch.bfloat16).to(torch.float32).numpy()
        reg = torch.from_numpy(reg).to(torch.bfloat16).to(torch.float32).numpy()
    return cls, reg


def _random_gt(rng, B, G, size=300.0):
    wh = rng.uniform(40, 220, (B, G, 2))
    xy = rng.uniform(0, 1, (B, G, 2)) * (size - wh)
    boxes = np.concatenate([xy, xy + wh], -1).astype(F)
    return boxes, rng.integers(0, NC, (B, G)).astype(np.int32)


def _small(name, boxes, labels, count, seed, G=None, cls_edit=None, expect=None):
    rng = np.random.default_rng(100 + seed)
    A = 12
    G = G or max(len(boxes), 1)
    gb, gl = np.zeros((1, G, 4), F), np.zeros((1, G), np.int32)
    for i, (bx, lb) in enumerate(zip(boxes, labels)):
        gb[0, i], gl[0, i] = bx, lb
    cls, reg = _logits(rng, 1, A)
    if cls_edit:
        cls_edit(cls)
    return dict(name=name, anchors='small', levels=SMALL_LEVELS, cls_strides=(20,), reg_strides=(8,), bf16=False, cls=cls, reg=reg,
                gt_boxes=gb, gt_labels=gl, gt_counts=np.asarray([count], np.int32), tie=cls_edit is not None, expect=expect)


def _dup_rows(cls):
    cls[0, 2:] = cls[0, 2]          # every negative but anchor 1 carries the same logits (anchor 0 is the positive)
    cls[0, 1] = cls[0, 2]


def small_cases():
    """The hand-worked cases (tests/test_ssd_loss_host.py spells the answers out)."""
    nan = float('nan')
    return [
        # the whole image: every 32 x 32 anchor has IoU 1024 / 6144 -- below 0.4, and the tie goes to anchor 0
        _small('contained', [[0, 0, 96, 64]], [3], 1, 0, expect=dict(positives={0: 0}, k=3)),
        # anchor 0 itself, then a box inside it whose best anchor is 0 as well: the later ground truth wins the anchor
        _small('shared', [[0, 0, 32, 32], [2, 2, 30, 30]], [1, 5], 2, 1, expect=dict(positives={0: 1}, k=3)),
        # overlaps nothing: maximum IoU 0 >= min_pos_iou 0, lowest anchor attaining it is 0 (restated, not repaired)
        _small('outside', [[1000, 1000, 1050, 1050]], [2], 1, 2, expect=dict(positives={0: 0}, k=3)),
        # NaN, x2 <= x1, label nc, label -1 are skipped; slot 4 (the cell of anchor 6) is the only ground truth
        _small('invalid', [[nan, 0, 32, 32], [40, 0, 40, 32], [0, 0, 32, 32], [32, 0, 64, 32], [0, 32, 32, 64]],
               [0, 1, NC, -1, 7], 5, 3, expect=dict(positives={6: 4}, k=3)),
        # four cells: 3 * 4 > 8 negatives, so every negative is mined
        _small('clamp', [[0, 0, 32, 32], [32, 0, 64, 32], [64, 0, 96, 32], [0, 32, 32, 64]], [0, 1, 2, 3], 4, 4,
               expect=dict(positives={0: 0, 2: 1, 4: 2, 6: 3}, k=8)),
        # eleven negatives with bit-equal logits: the three lowest indices are mined
        _small('tie', [[0, 0, 32, 32]], [4], 1, 5, cls_edit=_dup_rows, expect=dict(positives={0: 0}, k=3, mined=[1, 2, 3])),
        # no ground truth anywhere: avg = 1, everything 0
        _small('empty', [], [], 0, 0, expect=dict(positives={}, k=0)),
    ]


def _real(name, seed, bf16, cls_strides, reg_strides, B=3, G=8, counts=(0, 1, 8), levels=REAL_LEVELS):
    rng = np.random.default_rng(seed)
    A = 2044
    cls, reg = _logits(rng, B, A, bf16)
    gb, gl = _random_gt(rng, B, G)
    return dict(name=name, anchors='real', levels=levels, cls_strides=cls_strides, reg_strides=reg_strides, bf16=bf16, cls=cls,
                reg=reg, gt_boxes=gb, gt_labels=gl, gt_counts=np.asarray(counts, np.int32), tie=False, expect=None)


def _counts_case():
    """A count above G (clamped to G) and a negative count (clamped to 0), on the small anchors."""
    rng = np.random.default_rng(7)
    cls, reg = _logits(rng, 2, 12)
    gb = np.asarray([[[0, 0, 32, 32], [32, 32, 64, 64]], [[0, 0, 32, 32], [32, 32, 64, 64]]], F)
    gl = np.asarray([[1, 2], [3, 4]], np.int32)
    return dict(name='counts', anchors='small', levels=SMALL_LEVELS, cls_strides=(20,), reg_strides=(8,), bf16=False, cls=cls, reg=reg,
                gt_boxes=gb, gt_labels=gl, gt_counts=np.asarray([5, -2], np.int32), tie=False, expect=None)


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """Every case tests/test_gpu_ssd_loss.py runs through the kernel against this restatement (seeds 0-5)."""
    cases = small_cases()
    cases += [_real('real_fp32', 0, False, (40, 64), (16, 24)), _real('real_bf16', 1, True, (40, 64), (16, 24)),
              _real('real_fp32_wide', 2, False, (48, 72), (24, 32)), _real('real_bf16_wide', 3, True, (48, 72), (24, 32)),
              _counts_case(), _real('g_capacity', 4, False, (40, 64), (16, 24), B=1, G=64, counts=(64,)),
              _real('dense', 5, False, (10,), (4,), B=2, G=8, counts=(3, 8), levels=dict(hws=(2044,), nas=(1,)))]
    return tuple(cases)


def anchors_of(case):
    return small_anchors() if case['anchors'] == 'small' else real_anchors()


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    case = next(c for c in gpu_cases() if c['name'] == name)
    return multibox(case['cls'], case['reg'], anchors_of(case), case['gt_boxes'], case['gt_labels'], case['gt_counts'],
                    dtype=np.float32 if dtype == 'float32' else np.float64)


@functools.lru_cache(maxsize=None)
def spreads():
    """Largest float32-against-float64 difference of the restatement per output kind over all GPU cases."""
    out = dict(loss_cls=0.0, loss_bbox=0.0, dcls=0.0, dreg=0.0)
    for c in gpu_cases():
        r32, r64 = reference(c['name'], 'float32'), reference(c['name'], 'float64')
        assert (r32['assigned'] == r64['assigned']).all(), c['name']
        for k in ('loss_cls', 'loss_bbox'):
            out[k] = max(out[k], abs(r32[k] - r64[k]))
        for k in ('dcls', 'dreg'):
            out[k] = max(out[k], float(np.abs(r32[k].astype(np.float64) - r64[k]).max()))
    return out
