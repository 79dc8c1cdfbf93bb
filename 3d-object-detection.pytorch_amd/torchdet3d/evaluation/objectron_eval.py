"""The Objectron evaluation protocol of the reference's final report (`scripts/objectron_eval.py:116-237` around
`objectron.dataset.eval.Evaluator`) with the per-frame work on the device: `t3d_objectron_pairs` (match, lift, ground-plane
scale, pixel / azimuth / polar / 3-D IoU / ADD / ADD-S per predicted box) and `t3d_objectron_hitmiss` (instance count, hit /
miss at 21 thresholds per metric, partial sums), csrc/objectron_eval.hip.  `evaluate` only enqueues; the record stays on the
device until `finalize`, which reads it back once and computes VOC-style average precision on the host in fp64 numpy.

PARITY UNPINNED: `objectron.dataset.eval` / `objectron.dataset.metrics` are an empty submodule in the reference (SURVEY.md
appendix C).  DESIGN.md section 7 states the protocol; that statement is the definition.  Deviation: a non-finite metric
(a zero dot product in the scale, a singular viewpoint system) is carried, misses every threshold and is left out of the
means, where upstream would raise.  TFRecord parsing is out of scope: callers supply tensors.
"""
import numpy as np
import torch

from .. import _native as N

__all__ = ['ObjectronEvaluator', 'METRICS', 'make_thresholds', 'average_precision', 'finalize_record', 'format_report']

VIS, MAX_PIXEL, MAX_AZIMUTH, MAX_POLAR, MAX_DIST, NBINS = 0.1, 0.1, 30.0, 20.0, 1.0, 21
METRICS = ('pixel', 'azimuth', 'polar', 'iou', 'add', 'adds')        # the order of the device record
_HI = dict(pixel=MAX_PIXEL, azimuth=MAX_AZIMUTH, polar=MAX_POLAR, iou=1.0, add=MAX_DIST, adds=MAX_DIST)


def make_thresholds():
    """[6, 21] fp64 in `METRICS` order: numpy.linspace(0, hi, 21), computed here and uploaded (never on the device)."""
    return np.stack([np.linspace(0.0, _HI[m], NBINS) for m in METRICS])


def average_precision(hit, miss, total_instances):
    """VOC-style AP of one (metric, threshold): hit / miss [frames] in evaluation order."""
    tp, fp = np.cumsum(np.asarray(hit, np.float64)), np.cumsum(np.asarray(miss, np.float64))
    if len(tp) == 0 or total_instances <= 0:
        return 0.0
    recall = tp / float(total_instances)
    den = tp + fp
    precision = np.divide(tp, den, out=np.zeros_like(tp), where=den > 0)
    recall = np.concatenate([[0.0], recall, [1.0]])
    precision = np.concatenate([[0.0], precision, [0.0]])
    for i in range(len(precision) - 2, -1, -1):
        precision[i] = max(precision[i], precision[i + 1])
    idx = np.where(recall[:-1] != recall[1:])[0] + 1
    return float(np.sum((recall[idx] - recall[idx - 1]) * precision[idx]))


def finalize_record(valid, num_instances, hit, miss, sums):
    """Step 6 on the host: valid [R], num_instances [R], hit / miss [R, 6, 21], sums [R, 5] (error_2d, iou_3d, azimuth,
    polar, matched) -> the result dict of `ObjectronEvaluator.finalize`.  Rows with valid == 0 are dropped."""
    keep = np.asarray(valid).astype(bool)
    hit, miss = np.asarray(hit)[keep], np.asarray(miss)[keep]
    total = int(np.asarray(num_instances)[keep].sum())
    s = np.asarray(sums, np.float64)[keep].sum(0) if keep.any() else np.zeros(5)
    matched = int(round(s[4]))
    mean = lambda v: float(v / matched) if matched else 0.0        # noqa: E731
    thr = make_thresholds()
    aps = {m: np.array([average_precision(hit[:, i, j], miss[:, i, j], total) for j in range(NBINS)]) for i, m in enumerate(METRICS)}
    return dict(aps=aps, thresholds={m: thr[i] for i, m in enumerate(METRICS)}, error_2d=mean(s[0]), iou_3d=mean(s[1]),
                azimuth=mean(s[2]), polar=mean(s[3]), matched=matched, total_instances=total, frames=int(keep.sum()))


def format_report(res):
    """The text of the reference's report (objectron_eval.py:177-237): same lines, labels and number formats, with its
    `threshold * 0.1` on the pixel, azimuth and polar threshold rows."""
    def row(label, values, mul=1.0):
        return label + ''.join('{:.4f},\t'.format(v * mul) for v in values) + '\n'
    t, a = res['thresholds'], res['aps']
    out = 'Mean Error 2D: {}\n'.format(res['error_2d'])
    out += 'Mean 3D IoU: {}\n'.format(res['iou_3d'])
    out += 'Mean Azimuth Error: {}\n'.format(res['azimuth'])
    out += 'Mean Polar Error: {}\n'.format(res['polar'])
    out += '\n' + row('IoU Thresholds: ', t['iou']) + row('AP @3D IoU    : ', a['iou'])
    out += '\n' + row('2D Thresholds : ', t['pixel'], 0.1) + row('AP @2D Pixel  : ', a['pixel']) + '\n'
    out += row('Azimuth Thresh: ', t['azimuth'], 0.1) + row('AP @Azimuth   : ', a['azimuth']) + '\n'
    out += row('Polar Thresh  : ', t['polar'], 0.1) + row('AP @Polar     : ', a['polar']) + '\n'
    out += row('ADD Thresh    : ', t['add']) + row('AP @ADD       : ', a['add']) + '\n'
    out += row('ADDS Thresh   : ', t['adds']) + row('AP @ADDS      : ', a['adds'])
    return out


class ObjectronEvaluator:
    """`ObjectronEvaluator(max_frames, max_predictions, max_instances)`: a device record of `max_frames` rows, filled F rows
    at a time by `evaluate` / `evaluate_pipeline` (which never synchronise), read back once by `finalize`."""

    def __init__(self, max_frames, max_predictions, max_instances, device='cuda'):
        dev = torch.device(device)
        if dev.type != 'cuda' or not torch.cuda.is_available():
            raise RuntimeError('the Objectron evaluator runs on the GPU (no CPU fallback)')
        if min(int(max_frames), int(max_predictions), int(max_instances)) <= 0:
            raise ValueError('max_frames, max_predictions and max_instances must be positive')
        self.R, self.P, self.G = int(max_frames), int(max_predictions), int(max_instances)
        self.device = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        R, nb = self.R, len(METRICS) * NBINS
        # one block = one read-back: sums first (8-byte aligned), then the int32 sections
        self._layout, off = {}, 0
        for name, shape, dt in (('sums', (R, 5), torch.float64), ('hit', (R, len(METRICS), NBINS), torch.int32),
                                ('miss', (R, len(METRICS), NBINS), torch.int32), ('valid', (R,), torch.int32),
                                ('num_instances', (R,), torch.int32)):
            n = int(np.prod(shape)) * (8 if dt == torch.float64 else 4)
            self._layout[name] = (off, n, shape, dt)
            off += (n + 15) // 16 * 16
        assert self._layout['hit'][1] == R * nb * 4
        self._record = torch.zeros(off, dtype=torch.uint8, device=self.device)
        self._host = torch.zeros(off, dtype=torch.uint8).pin_memory()
        self._r = self._views(self._record)
        self._thr = torch.from_numpy(make_thresholds()).to(self.device)
        self._scratch = {}
        self.base = 0
        self._result = None
        self._done = torch.cuda.Event()          # recorded behind every evaluate: finalize's read-back waits for it

    def _views(self, block):
        return {k: block[o:o + n].view(dt).view(shape) for k, (o, n, shape, dt) in self._layout.items()}

    def reset(self):
        self.base, self._result = 0, None

    # ---- one batch of frames -------------------------------------------------------------------------------------------------
    def _check(self, t, name, shape, dtype=torch.float64):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f'{name} must be a device tensor (no CPU fallback)')
        if t.device != self.device:
            raise ValueError(f'{name} on {t.device}, the evaluator on {self.device}')
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {tuple(shape)}')
        return t.to(dtype).contiguous()

    def evaluate(self, pred_kp, pred_count, gt_kp2d, gt_kp3d, gt_visibility, gt_count, planes, frame_size=None):
        """Appends F rows.  pred_kp [F,P,9,2] (or [F,P,18]) keypoints normalised to the frame -- or frame pixels with
        frame_size = (W, H); pred_count [F]; gt_kp2d [F,G,9,2] normalised; gt_kp3d [F,G,9,3]; gt_visibility [F,G];
        gt_count [F]; planes [F,6] (centre, normal).  P <= max_predictions, G <= max_instances.  Floating tensors are taken
        as fp64, counts as int32 (converted on the device when they are not).  Never synchronises.
        Returns (metrics [F,P,6] fp64 in `METRICS` order, matched [F,P] int32): the per-slot results, device views of the
        evaluator's scratch, valid until the next call (slots at or past pred_count[f] are stale).
        Not replayable: the row `base` is a literal word of the launch and advances on the host, so a `PlanRecorder` that
        captured this call would write the same rows again at every replay -- call `evaluate` itself once per batch (the two
        entry points are recordable by a caller that manages `base` on its own)."""
        for name, t in (('pred_kp', pred_kp), ('gt_kp2d', gt_kp2d)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f'{name} must be a device tensor (no CPU fallback)')
        if pred_kp.dim() < 2 or gt_kp2d.dim() < 2:
            raise ValueError('pred_kp must be [F,P,9,2] and gt_kp2d [F,G,9,2]')
        F, P, G = int(pred_kp.shape[0]), int(pred_kp.shape[1]), int(gt_kp2d.shape[1])
        if F <= 0 or not 0 < P <= self.P or not 0 < G <= self.G:
            raise ValueError(f'F = {F}, P = {P}, G = {G}: the evaluator holds up to P = {self.P}, G = {self.G}')
        if pred_kp.dim() == 3 and pred_kp.shape[2] == 18:
            pred_kp = pred_kp.reshape(F, P, 9, 2)
        pred_kp = self._check(pred_kp, 'pred_kp', (F, P, 9, 2))
        pred_count = self._check(pred_count, 'pred_count', (F,), torch.int32)
        gt_kp2d = self._check(gt_kp2d, 'gt_kp2d', (F, G, 9, 2))
        gt_kp3d = self._check(gt_kp3d, 'gt_kp3d', (F, G, 9, 3))
        gt_visibility = self._check(gt_visibility, 'gt_visibility', (F, G))
        gt_count = self._check(gt_count, 'gt_count', (F,), torch.int32)
        planes = self._check(planes.reshape(planes.shape[0], -1) if torch.is_tensor(planes) else planes, 'planes', (F, 6))
        if self.base + F > self.R:
            raise ValueError(f'the record is full: {self.base} of {self.R} rows used, {F} more asked for')
        sx, sy = (1.0, 1.0) if frame_size is None else (1.0 / float(frame_size[0]), 1.0 / float(frame_size[1]))
        key = (F, P)
        if key not in self._scratch:
            self._scratch = {key: (torch.zeros(F, P, 6, dtype=torch.float64, device=self.device),
                                   torch.zeros(F, P, dtype=torch.int32, device=self.device))}
        metrics, matched = self._scratch[key]
        with torch.cuda.device(self.device):
            st, r = N.stream(), self._r
            N.call('t3d_objectron_pairs', N.ptr(pred_kp), N.ptr(pred_count), N.ptr(gt_kp2d), N.ptr(gt_kp3d), N.ptr(gt_visibility),
                   N.ptr(gt_count), N.ptr(planes), F, P, G, sx, sy, N.ptr(metrics), N.ptr(matched), st)
            N.call('t3d_objectron_hitmiss', N.ptr(metrics), N.ptr(matched), N.ptr(pred_count), N.ptr(gt_kp2d), N.ptr(gt_kp3d),
                   N.ptr(gt_visibility), N.ptr(gt_count), N.ptr(self._thr), F, P, G, self.base, self.R, N.ptr(r['valid']),
                   N.ptr(r['num_instances']), N.ptr(r['hit']), N.ptr(r['miss']), N.ptr(r['sums']), st)
            self._done.record(torch.cuda.current_stream(self.device))
        self.base += F
        self._result = None
        return metrics, matched

    def evaluate_pipeline(self, result, gt_kp2d, gt_kp3d, gt_visibility, gt_count, planes, frame_size):
        """`FramePipeline.process_device`'s dict: every camera is a frame, kp_frame [S,T,18] (frame pixels) are its predictions
        and count [S] their number; frame_size = (W, H)."""
        return self.evaluate(result['kp_frame'], result['count'], gt_kp2d, gt_kp3d, gt_visibility, gt_count, planes,
                             frame_size=frame_size)

    # ---- the end ---------------------------------------------------------------------------------------------------------------
    def finalize(self):
        """One read-back of the record, invalid rows dropped, average precision per metric and threshold over the frames in
        the order they were evaluated: dict(aps {metric: [21]}, thresholds {metric: [21]}, error_2d, iou_3d, azimuth,
        polar (means over the matched predictions), matched, total_instances, frames)."""
        if self._result is None:
            with torch.cuda.device(self.device):
                torch.cuda.current_stream().wait_event(self._done)      # evaluate may have run on another stream
                self._host.copy_(self._record, non_blocking=True)
                torch.cuda.current_stream().synchronize()
            h = {k: v[:self.base].numpy() for k, v in self._views(self._host).items()}
            self._result = finalize_record(h['valid'], h['num_instances'], h['hit'], h['miss'], h['sums'])
        return self._result

    def write_report(self, path):
        with open(path, 'w') as f:
            f.write(format_report(self.finalize()))
