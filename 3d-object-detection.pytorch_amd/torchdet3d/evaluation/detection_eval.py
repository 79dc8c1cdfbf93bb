"""COCO bbox evaluation of the detector's validation (`CocoDataset.evaluate(metric='bbox')` of mmdet 2.x around pycocotools'
`COCOeval`, what `configs/detection/mnv2_ssd_300_2_heads.py:56-60,130-143` of the reference asks for) with the per-image
work on the device: `t3d_ssd_cap_per_image` (test_cfg.max_per_img) and `t3d_coco_match` (rescale to the original frame,
IoU, the greedy matching at 4 area ranges x 10 thresholds), csrc/detection_eval.hip.  `evaluate` only enqueues; the record
stays on the device until `finalize`, which reads it back once and runs `COCOeval.accumulate` / `summarize` on the host in
fp64 numpy.

PARITY UNPINNED: `pycocotools` and `mmdet` are not installed where this project is built.  DESIGN.md section 7 states the
protocol; that statement is the definition, tests/coco_eval_ref.py is its plain-loop form.  Deviations: no crowd branch (the
reference's converter writes iscrowd = 0 everywhere and the loader drops crowd boxes), NMS at input scale before the rescale
(mmdet rescales first), no xywh round trip through a JSON result file.
"""
import numpy as np
import torch

from .. import _native as N

__all__ = ['DetectionEvaluator', 'make_iou_thresholds', 'make_rec_thresholds', 'make_area_ranges', 'accumulate', 'summarize',
           'report', 'MAX_DETS', 'AREA_NAMES', 'MAX_GT']

MAX_DETS = (1, 10, 100)
AREA_NAMES = ('all', 'small', 'medium', 'large')
MAX_GT = 64                 # t3d_coco_match: a cell's IoU matrix lives in LDS
_ND = MAX_DETS[-1]


def make_iou_thresholds():
    """[10] fp64, COCOeval's `np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1)`; computed here, uploaded."""
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def make_rec_thresholds():
    """[101] fp64, COCOeval's `np.linspace(.0, 1.00, 101)`."""
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def make_area_ranges():
    """[4, 2] fp64 (lo, hi) in `AREA_NAMES` order, both ends inclusive."""
    return np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)


def accumulate(score, dtm, dtig, ndt, ngt, valid=None):
    """`COCOeval.accumulate` over the record, rows in evaluation order: score [R,nc,100] fp32, dtm / dtig [R,nc,100] uint64
    (bit a * 10 + t), ndt [R,nc], ngt [R,nc,4] (non-ignored ground truths per area range), valid [R] (rows with 0 are
    dropped) -> precision [10,101,nc,4,3], recall [10,nc,4,3], -1 where a (class, area range) has no ground truth."""
    score, dtm, dtig = np.asarray(score, np.float32), np.asarray(dtm, np.uint64), np.asarray(dtig, np.uint64)
    ndt, ngt = np.asarray(ndt, np.int64), np.asarray(ngt, np.int64)
    if valid is not None:
        keep = np.asarray(valid).astype(bool)
        score, dtm, dtig, ndt, ngt = score[keep], dtm[keep], dtig[keep], ndt[keep], ngt[keep]
    nc = ndt.shape[1]
    rec_thrs = make_rec_thresholds()
    T, A, M, nr = len(make_iou_thresholds()), len(AREA_NAMES), len(MAX_DETS), len(rec_thrs)
    precision, recall = -np.ones((T, nr, nc, A, M)), -np.ones((T, nc, A, M))
    slot = np.arange(_ND)[None, :]
    eps = np.spacing(1)
    for k in range(nc):
        for m, max_det in enumerate(MAX_DETS):
            sel = slot < np.minimum(ndt[:, k], max_det)[:, None]       # image-major, then the cell's own order
            sc = score[:, k][sel]
            inds = np.argsort(-sc, kind='mergesort')
            wm, wi = dtm[:, k][sel][inds], dtig[:, k][sel][inds]
            nd = len(inds)
            for a in range(A):
                npig = int(ngt[:, k, a].sum())
                if npig == 0:
                    continue
                bits = (a * T + np.arange(T, dtype=np.uint64))[:, None]
                hit = ((wm[None, :] >> bits) & np.uint64(1)).astype(bool)
                ign = ((wi[None, :] >> bits) & np.uint64(1)).astype(bool)
                tp_sum = np.cumsum(hit & ~ign, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~hit & ~ign, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + eps)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]          # the backward precision envelope
                    at = np.searchsorted(rc, rec_thrs, side='left')
                    q = np.zeros(nr)
                    q[at < nd] = pr[at[at < nd]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall):
    """`COCOeval.summarize`'s twelve numbers: AP, AP50, AP75, AP small / medium / large (maxDets 100), AR at maxDets 1, 10,
    100, AR small / medium / large; each the mean over the entries > -1, or -1 when there is none."""
    thrs = make_iou_thresholds()

    def one(ap, iou=None, area=0, m=len(MAX_DETS) - 1):
        s = precision[:, :, :, area, m] if ap else recall[:, :, area, m]
        if iou is not None:
            s = s[np.where(iou == thrs)[0]]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return np.array([one(1), one(1, .5), one(1, .75), one(1, area=1), one(1, area=2), one(1, area=3),
                     one(0, m=0), one(0, m=1), one(0, m=2), one(0, area=1), one(0, area=2), one(0, area=3)])


def report(precision, recall, classes, images):
    """The dict `DetectionEvaluator.finalize` returns: mmdet's keys (three decimals) and the unrounded arrays."""
    stats = summarize(precision, recall)
    res = {'bbox_' + k: float(f'{v:.3f}') for k, v in zip(('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l'), stats)}
    res['bbox_mAP_copypaste'] = ' '.join(f'{v:.3f}' for v in stats[:6])
    classwise = {}
    for k, name in enumerate(classes):
        p = precision[:, :, k, 0, -1]
        p = p[p > -1]
        classwise[name] = float(np.mean(p)) if p.size else float('nan')
    res.update(stats=stats, precision=precision, recall=recall, classwise=classwise, images=int(images))
    return res


class DetectionEvaluator:
    """`DetectionEvaluator(detector, max_images)`: a device record of `max_images` rows, filled B rows at a time by `evaluate`
    / `evaluate_detections` (which never synchronise), read back once by `finalize`.  `detector`: an `SSD300` (its
    `detect_device`, class count and `max_per_img` are used) -- or None for `evaluate_detections` alone, with `num_classes`
    and `max_per_img` given."""

    def __init__(self, detector, max_images, device='cuda', num_classes=None, max_per_img=None, classes=None):
        dev = torch.device(device)
        if dev.type != 'cuda' or not torch.cuda.is_available():
            raise RuntimeError('the detection evaluator runs on the GPU (no CPU fallback)')
        if int(max_images) <= 0:
            raise ValueError('max_images must be positive')
        self.detector = detector
        self.nc = int(detector.nc if num_classes is None else num_classes)
        self.max_per_img = int(detector.max_per_img if max_per_img is None else max_per_img)
        if self.nc <= 0 or self.max_per_img < 0:
            raise ValueError('num_classes must be positive and max_per_img non-negative')
        if classes is None:
            from ..models.ssd import CLASSES
            classes = CLASSES if len(CLASSES) == self.nc else tuple(str(k) for k in range(self.nc))
        if len(classes) != self.nc:
            raise ValueError(f'{len(classes)} class names for {self.nc} classes')
        self.classes = tuple(classes)
        self.R = int(max_images)
        self.device = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        R, nc = self.R, self.nc
        # one block = one mirror: the 8-byte sections first
        self._layout, off = {}, 0
        for name, shape, dt in (('dtm', (R, nc, _ND), torch.int64), ('dtig', (R, nc, _ND), torch.int64),
                                ('score', (R, nc, _ND), torch.float32), ('ndt', (R, nc), torch.int32),
                                ('ngt', (R, nc, len(AREA_NAMES)), torch.int32), ('valid', (R,), torch.int32)):
            n = int(np.prod(shape)) * (8 if dt == torch.int64 else 4)
            self._layout[name] = (off, n, shape, dt)
            off += (n + 15) // 16 * 16
        self._record = torch.zeros(off, dtype=torch.uint8, device=self.device)
        self._host = torch.zeros(off, dtype=torch.uint8).pin_memory()
        self._r = self._views(self._record)
        self._thr = torch.from_numpy(make_iou_thresholds()).to(self.device)
        self._rng = torch.from_numpy(make_area_ranges()).to(self.device)
        self._capped = {}
        self.base = 0
        self._result = None
        self._done = torch.cuda.Event()          # recorded behind every evaluate: finalize's read-back waits for it

    def _views(self, block):
        return {k: block[o:o + n].view(dt).view(shape) for k, (o, n, shape, dt) in self._layout.items()}

    def reset(self):
        self.base, self._result = 0, None

    # ---- one batch of images -------------------------------------------------------------------------------------------------
    def _check(self, t, name, shape, dtype):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f'{name} must be a device tensor (no CPU fallback)')
        if t.device != self.device:
            raise ValueError(f'{name} on {t.device}, the evaluator on {self.device}')
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {tuple(shape)}')
        return t.to(dtype).contiguous()

    def evaluate_detections(self, out, cnt, gt_boxes, gt_labels, gt_counts, ori_shapes, input_size=None):
        """Appends B rows for detections the caller already holds: out [B,nc,K,6] fp32 / cnt [B,nc] int32 as
        `SSD300.detect_device` leaves them (boxes in input pixels, the rows of a class in non-increasing score order);
        gt_boxes [B,G,4] fp32 in input pixels, gt_labels [B,G] int32, gt_counts [B] int32, ori_shapes [B,2] int32 = (h, w)
        of each original frame -- what the `val` loader yields; input_size = (h, w) of the network input (default: the
        detector's).  G <= 64.  Applies max_per_img (`out` and `cnt` are left as they are), then matches.  Never
        synchronises.  Returns the capped counts [B,nc] int32, a device view of the evaluator's scratch, valid until the
        next call at this batch size.
        Not replayable: the row `base` is a literal word of the launch and advances on the host, so a `PlanRecorder` that
        captured this call would write the same rows again at every replay -- call it once per batch (the two entry points
        are recordable by a caller that manages `base` on its own)."""
        for name, t in (('out', out), ('gt_boxes', gt_boxes)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f'{name} must be a device tensor (no CPU fallback)')
        if out.dim() != 4 or gt_boxes.dim() != 3:
            raise ValueError('out must be [B,nc,K,6] and gt_boxes [B,G,4]')
        B, K, G = int(out.shape[0]), int(out.shape[2]), int(gt_boxes.shape[1])
        if B <= 0 or K <= 0 or G > MAX_GT:
            raise ValueError(f'B = {B}, K = {K}, G = {G}: the evaluator takes B >= 1, K >= 1 and G <= {MAX_GT}')
        out = self._check(out, 'out', (B, self.nc, K, 6), torch.float32)
        cnt = self._check(cnt, 'cnt', (B, self.nc), torch.int32)
        gt_boxes = self._check(gt_boxes, 'gt_boxes', (B, G, 4), torch.float32)
        gt_labels = self._check(gt_labels, 'gt_labels', (B, G), torch.int32)
        gt_counts = self._check(gt_counts, 'gt_counts', (B,), torch.int32)
        ori_shapes = self._check(ori_shapes, 'ori_shapes', (B, 2), torch.int32)
        if input_size is None:
            from ..models.ssd import INPUT_SIZE
            input_size = (INPUT_SIZE, INPUT_SIZE)
        in_h, in_w = int(input_size[0]), int(input_size[1])
        if in_h <= 0 or in_w <= 0:
            raise ValueError(f'input_size = {tuple(input_size)} must be positive')
        if self.base + B > self.R:
            raise ValueError(f'the record is full: {self.base} of {self.R} rows used, {B} more asked for')
        if B not in self._capped:
            self._capped[B] = torch.zeros(B, self.nc, dtype=torch.int32, device=self.device)
        capped = self._capped[B]
        with torch.cuda.device(self.device):
            st, r = N.stream(), self._r
            N.call('t3d_ssd_cap_per_image', N.ptr(out), N.ptr(cnt), B, self.nc, K, self.max_per_img, N.ptr(capped), st)
            N.call('t3d_coco_match', N.ptr(out), N.ptr(capped), B, self.nc, K, N.ptr(gt_boxes) if G else None,
                   N.ptr(gt_labels) if G else None, N.ptr(gt_counts), G, N.ptr(ori_shapes), in_w, in_h, N.ptr(self._thr),
                   N.ptr(self._rng), self.base, self.R, N.ptr(r['score']), N.ptr(r['dtm']), N.ptr(r['dtig']), N.ptr(r['ndt']),
                   N.ptr(r['ngt']), N.ptr(r['valid']), st)
            self._done.record(torch.cuda.current_stream(self.device))
        self.base += B
        self._result = None
        return capped

    def evaluate(self, imgs, gt_boxes, gt_labels, gt_counts, ori_shapes):
        """One batch of the `val` loader: `detector.detect_device(imgs)` (imgs uint8 [B,oh,ow,3]; the engine's inference
        path, which folds the running BatchNorm estimates as they stand at every call -- after a training step too), then
        `evaluate_detections` with input_size = (oh, ow).  Appends B rows, never synchronises, not replayable (see
        `evaluate_detections`)."""
        if self.detector is None:
            raise RuntimeError('this evaluator was built without a detector: call evaluate_detections')
        if not torch.is_tensor(imgs) or not imgs.is_cuda:
            raise RuntimeError('imgs must be a device tensor (no CPU fallback)')
        if imgs.device != self.device:
            raise ValueError(f'imgs on {imgs.device}, the evaluator on {self.device}')
        if imgs.dim() != 4 or imgs.dtype != torch.uint8 or imgs.shape[3] != 3:
            raise ValueError(f'imgs must be uint8 [B,oh,ow,3], got {imgs.dtype} {tuple(imgs.shape)}')
        if self.base + int(imgs.shape[0]) > self.R:
            raise ValueError(f'the record is full: {self.base} of {self.R} rows used, {int(imgs.shape[0])} more asked for')
        with torch.cuda.device(self.device):
            out, cnt = self.detector.detect_device(imgs)
        return self.evaluate_detections(out, cnt, gt_boxes, gt_labels, gt_counts, ori_shapes,
                                        input_size=(int(imgs.shape[1]), int(imgs.shape[2])))

    def val(self, loader):
        """One validation epoch: `reset`, `evaluate` over every batch of `loader` (a `val` loader of
        `build_detection_loader`) with nothing read back per batch, then `finalize`.  Nothing has to be switched on the
        detector between a training step and this: `detect_device` runs the engine's inference pass."""
        self.reset()
        for batch in loader:
            self.evaluate(*batch[:5])
        return self.finalize()

    # ---- the end ---------------------------------------------------------------------------------------------------------------
    def record(self):
        """One read-back: the first `base` rows of every section of the record as numpy arrays (dtm / dtig as uint64)."""
        n = self.base
        host = self._views(self._host)
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().wait_event(self._done)      # evaluate may have run on another stream
            if n:
                for k, v in self._r.items():
                    host[k][:n].copy_(v[:n], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        h = {k: v[:n].numpy().copy() for k, v in host.items()}
        h['dtm'], h['dtig'] = h['dtm'].view(np.uint64), h['dtig'].view(np.uint64)
        return h

    def finalize(self):
        """One read-back of the record, then `accumulate` / `summarize` over the images in the order they were evaluated:
        dict(bbox_mAP, bbox_mAP_50, bbox_mAP_75, bbox_mAP_s, bbox_mAP_m, bbox_mAP_l (each float(f'{v:.3f}')),
        bbox_mAP_copypaste, stats [12] unrounded, precision [10,101,nc,4,3], recall [10,nc,4,3], classwise {name: AP},
        images)."""
        if self._result is None:
            h = self.record()
            precision, recall = accumulate(h['score'], h['dtm'], h['dtig'], h['ndt'], h['ngt'], h['valid'])
            self._result = report(precision, recall, self.classes, int(h['valid'].astype(bool).sum()))
        return self._result
