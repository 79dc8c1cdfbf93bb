"""The live pipeline of `scripts/demo.py:56-78` -- detector -> regressor -> tracker -> keypoints in frame pixels -- as ONE
device-resident chain per frame, for S cameras at once.

The stages are the product's own (`Detector`, `Regressor`, `IOUTracker`); what this module adds are the joints, which used
to be host code with a read-back each: `t3d_ssd_select_rects` (the detector's class merge, score threshold, pixel boxes,
sort and cap -- `SSD300.detect` + `Detector._decode_detections`), `t3d_head_select` (the arg-max class's head) and
`t3d_track_kp_to_frame` (`Regressor.transform_kp` per tracked object), csrc/pipeline.hip.  `process_device` enqueues the
chain and never synchronises; after the warm-up frames the chain is recorded once (`PlanRecorder`, like
trainer/step_plan.py: ForwardPlan) and every later frame is one `t3d_plan_run` with the frames' address as its slot.

Deviations from the reference's loop: at most D = `tracker.max_detections` detections per frame and camera go on (the
reference's lists are unbounded; `overflow` counts what the cap dropped), the regressor always runs on D crops per camera
(rows past the count are black crops whose results nothing reads), and the regressor sees the SAME frame's detections (the
reference overlaps the detector with the previous frame's regression on the host, one frame of lag between them).
"""
import ctypes
import os

import numpy as np
import torch

from .. import _native as N
from ..trainer.step_plan import WARM_STEPS
from .draw import DrawStyle
from .tracking_tools import TrackedObj

__all__ = ['FramePipeline']


def _resolved(dev):
    dev = torch.device(dev)
    return torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index) if dev.type == 'cuda' else dev


class FramePipeline:
    """`FramePipeline(detector, regressor, tracker, draw=None)`: S = `tracker.streams` cameras, D = `tracker.max_detections`.
    `replays` counts the frames that ran as one `t3d_plan_run` (T3D_STEP_PLAN=0 keeps the launch-by-launch form).
    `draw`: a `DrawStyle` -- the chain then ends with the demo's `draw_detections` (scripts/demo.py:79-81) as one more launch:
    the tracked objects' rectangles, boxes, keypoints and class names are drawn on `frames` IN PLACE (utils/draw.py; the look
    is unpinned against the reference's).  None (default): the frames are left as they are."""

    def __init__(self, detector, regressor, tracker, draw=None):
        if not torch.cuda.is_available():
            raise RuntimeError('the frame pipeline runs on the GPU (no CPU fallback)')
        self.device = _resolved(detector.device)
        if _resolved(regressor.device) != self.device or _resolved(tracker.device) != self.device:
            raise ValueError(f'detector on {self.device}, regressor on {regressor.device}, tracker on {tracker.device}: '
                             'the stages of one pipeline share a device')
        self.detector, self.regressor, self.tracker = detector, regressor, tracker
        self.S, self.D, self.T = tracker.streams, tracker.max_detections, tracker.max_tracks
        self.rec, self.key, self.warm, self.replays = None, None, 0, 0
        self.replay = os.environ.get('T3D_STEP_PLAN', '1') != '0'      # read here: 0 keeps this pipeline launch by launch
        self.slots = (ctypes.c_ulonglong * N.NSLOTS)()
        self._block = None
        if draw is not None and not isinstance(draw, DrawStyle):
            raise ValueError('draw must be a DrawStyle or None')
        self.draw = draw
        self._style = draw.pack() if draw is not None else None       # (copied into the launch, and into a recorded plan)

    # ---- buffers ---------------------------------------------------------------------------------------------------------
    def _allocate(self):
        """One block: the tracker's outputs (moved here, so that everything a frame yields is one read-back) followed by the
        pipeline's own; every section 16-byte aligned."""
        S, D, T, tr = self.S, self.D, self.T, self.tracker
        tr._ensure()
        sizes = [('kp_frame', (S, T, 18), torch.float64), ('counts', (S,), torch.int32), ('overflow', (S,), torch.int32),
                 ('rects', (S, D, 4), torch.int32), ('crop_rects', (S * D, 4), torch.int32), ('scores', (S, D), torch.float32),
                 ('det_labels', (S, D), torch.int32), ('labels', (S, D), torch.int32), ('kp', (S, D, 18), torch.float32)]
        layout, off = [], tr._out_bytes
        for name, shape, dt in sizes:
            nb = int(np.prod(shape)) * (8 if dt == torch.float64 else 4)
            layout.append((name, shape, dt, off, nb))
            off += (nb + 15) // 16 * 16
        self._layout = layout
        self._block = torch.zeros(off, dtype=torch.uint8, device=self.device)
        self._host = torch.zeros(off, dtype=torch.uint8).pin_memory()
        self._block[:tr._out_bytes].copy_(tr._out)
        tr._out = self._block[:tr._out_bytes]
        tr._o = tr._views(tr._out)
        self._o = tr._views(self._block, layout)
        self._h = {('track_kp' if k == 'kp' else k): v for k, v in tr._views(self._host[:tr._out_bytes]).items()}
        self._h.update(tr._views(self._host, layout))

    def _shape_buffers(self, S, H, W):
        from ..models.ssd import INPUT_SIZE
        ys = torch.arange(S, dtype=torch.int32) * H
        self._frame_rects = torch.stack([torch.zeros_like(ys), ys, torch.full_like(ys, W), ys + H], 1).contiguous().to(self.device)
        self._imgs = torch.empty(S, INPUT_SIZE, INPUT_SIZE, 3, dtype=torch.uint8, device=self.device)

    # ---- the chain -----------------------------------------------------------------------------------------------------------
    def _chain(self, frames, S, H, W):
        from ..models.ssd import INPUT_SIZE
        det, reg, tr, o, st = self.detector, self.regressor, self.tracker, self._o, N.stream()
        m, D = det.model, self.D
        # the S frames are one tall frame to the resize kernel (Detector.get_detections_batch)
        N.call('t3d_crop_resize_u8', N.ptr(frames), N.ptr(self._frame_rects), N.ptr(self._imgs), S, S * H, W, INPUT_SIZE, INPUT_SIZE, st)
        out, cnt = m.detect_device(self._imgs)
        N.call('t3d_ssd_select_rects', N.ptr(out), N.ptr(cnt), S, m.nc, m.max_per_img, m.max_per_img, float(INPUT_SIZE),
               float(det.confidence), H, W, float(det.expand_ratio[0]), float(det.expand_ratio[1]), D, N.ptr(o['rects']),
               N.ptr(o['crop_rects']), N.ptr(o['scores']), N.ptr(o['det_labels']), N.ptr(o['counts']), N.ptr(o['overflow']), st)
        reg.regress_device(frames, o['crop_rects'], S * D, out=(o['kp'].view(S * D, 18), o['labels'].view(S * D)))
        tr.process_batch_device(o['rects'], o['kp'], o['counts'])
        t = tr._o
        N.call('t3d_track_kp_to_frame', N.ptr(t['count']), N.ptr(t['boxes']), N.ptr(t['kp']), N.ptr(o['kp_frame']), S, self.T, st)
        if self._style is not None:
            # scripts/demo.py:79: the tracked objects zipped in index order with the regressor's outputs (their labels).  The
            # launch reads kp_frame, the chain's last product, so it is behind every reader of the frames it draws on
            N.call('t3d_draw_overlays_u8', N.ptr(frames), S, H, W, N.ptr(t['count']), N.ptr(t['boxes']), N.ptr(o['kp_frame']),
                   N.ptr(t['ids']), N.ptr(o['labels']), N.ptr(o['counts']), D, self.T, self._style, st)

    def _results(self):
        o, t = self._o, self.tracker._o
        res = {k: o[k] for k in ('counts', 'rects', 'scores', 'det_labels', 'overflow', 'labels', 'kp', 'kp_frame')}
        res.update({('track_kp' if k == 'kp' else k): v for k, v in t.items()})
        return res

    def process_device(self, frames):
        """frames [S,H,W,3] uint8 on the device ([H,W,3] when S == 1).  Enqueues one frame of every camera and returns a dict
        of device views, valid until the next call: counts [S], rects [S,D,4], scores [S,D], det_labels [S,D], overflow [S]
        (the detector's rows, zeros past counts), labels [S,D] int32 and kp [S,D,18] (crop-normalised, of the arg-max head),
        everything `IOUTracker.tracked_device()` returns under its own names (count, boxes, ids, scalars) except the tracked
        keypoints [S,T,18] float64, which are `track_kp` here (`kp` is the regressor's), and kp_frame [S,T,18] float64 (the
        tracked keypoints in frame pixels).  With `draw` set, `frames` carries the overlays afterwards.  Never synchronises."""
        S = self.S
        if frames.dim() == 3 and S == 1:
            frames = frames.unsqueeze(0)
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[0] == S and frames.shape[3] == 3):
            raise ValueError(f'frames must be a uint8 device tensor [{S}, H, W, 3]')
        if _resolved(frames.device) != self.device:
            raise ValueError(f'frames on {frames.device}, the pipeline on {self.device}')
        if self._style is not None and not frames.is_contiguous():
            raise ValueError('frames must be contiguous: the overlays are drawn on them in place')
        frames = frames.contiguous()
        H, W = int(frames.shape[1]), int(frames.shape[2])
        if self._block is None:
            self._allocate()
        # (the detector's threshold / expand ratio and the tracker's settings are literal words of a recorded plan: a change
        # of any of them is a new plan too)
        key = (S, H, W, frames.dtype, N.stream(), float(self.detector.confidence), tuple(self.detector.expand_ratio), self._tracker_settings(),
               bytes(self._style) if self._style is not None else None)
        if key != self.key:
            self.drop()
            self._shape_buffers(S, H, W)
            self.key, self.warm = key, 0
        # weights are packed outside the plan (they may have moved since the last frame)
        m = self.detector.model
        m.backbone._pack()
        if m._packed is None:
            m._pack()
        self.regressor.model.net_eval._pack()
        if self.rec is not None:
            self.slots[N.SLOT_IMGS] = frames.data_ptr()
            rc = N.lib().t3d_plan_run(self.rec.plan, 0, self.slots, N.NSLOTS, None, 0)
            if rc < 0:
                code = ctypes.c_int(0)
                op = N.lib().t3d_plan_failed_op(self.rec.plan, ctypes.byref(code))
                raise RuntimeError(f't3d_plan_run failed at op {op} with code {code.value}')
            self.replays += 1
            return self._results()
        rec = None
        if self.replay and N.timer is None and N.recorder is None and self.warm >= WARM_STEPS:
            rec = N.PlanRecorder({frames.data_ptr(): N.SLOT_IMGS})
            N.recorder = rec
        try:
            self._chain(frames, S, H, W)
            if rec is not None:
                rec.end_segment()
                rec.keep += [self._block, self._frame_rects, self._imgs, self.tracker._state]
        except BaseException:
            if rec is not None:
                rec.close()
            raise
        finally:
            if rec is not None:
                N.recorder = None
        self.warm += 1
        if rec is not None:
            if rec.broken or rec.breaks:
                rec.close()
                self.warm = -(1 << 30)            # stays launch by launch at this shape
            else:
                self.rec = rec
        return self._results()

    def _tracker_settings(self):
        t = self.tracker
        return (t.time_window, t.continue_time_thresh, t.track_clear_thresh, t.match_threshold, t.track_detection_iou_thresh,
                t.interpolate_time_thresh, t.detection_filter_speed, t.keypoints_filter_speed, t.add_treshold,
                t.no_updated_frames_treshold, bool(t.align_kp))

    def drop(self):
        if self.rec is not None:
            self.rec.close()
            self.rec = None

    def __del__(self):
        try:
            self.drop()
        except Exception:       # noqa: BLE001
            pass

    # ---- the demo's host view ------------------------------------------------------------------------------------------------
    def process(self, frame):
        """One frame of a single-camera pipeline (ndarray [H,W,3] uint8 or a device tensor) -> (detections, outputs, tracked,
        decoded_kps): the four lists of scripts/demo.py:67-78 -- the detector's (left, top, right, bottom, confidence, label)
        tuples, the regressor's (kp ndarray [1,9,2], label) pairs, the tracker's `TrackedObj`s and their keypoints in frame
        pixels ([9,2] float64 each) -- from one pinned read-back and one synchronisation."""
        if self.S != 1:
            raise ValueError('process addresses a single-camera pipeline; use process_device')
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        frame = frame.to(self.device, non_blocking=True)
        self.process_device(frame)
        self._host.copy_(self._block, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        h = self._h
        n = int(h['counts'][0])
        rects, scores, dl = h['rects'][0, :n].tolist(), h['scores'][0, :n].tolist(), h['det_labels'][0, :n].tolist()
        detections = [(*rects[i], scores[i], dl[i]) for i in range(n)]
        kp, labels = h['kp'][0, :n].numpy().copy().reshape(n, 1, 9, 2), h['labels'][0, :n].tolist()
        outputs = [(kp[i], labels[i]) for i in range(n)]
        nt = int(h['count'][0])
        boxes, tkp, ids = h['boxes'][0, :nt].tolist(), h['track_kp'][0, :nt].tolist(), h['ids'][0, :nt].tolist()
        tracked = [TrackedObj(tuple(boxes[i]), tuple(tkp[i]), f'ID {ids[i]}') for i in range(nt)]
        kpf = h['kp_frame'][0, :nt].numpy().copy().reshape(nt, 9, 2)
        return detections, outputs, tracked, [kpf[i] for i in range(nt)]
