"""Third stage of the demo pipeline on the HIP path: the IOU tracker, resident on the device.

Mirrors the reference's `torchdet3d/utils/tracking_tools.py` (`IOUTracker`, :127-290; call site scripts/demo.py:56-78):
`tracker.process(frame, detections, kps)` then `tracker.get_tracked_objects()` keep their meaning, but the whole tracker
state -- per track the last box, the last keypoints, end time, length, `no_updated_frames`, plus the id FIFO and the
counters -- lives in HBM, and a frame is ONE launch of `t3d_track_step` (csrc/track.hip) for all streams: active tracks,
GIoU cost matrix, minimum-cost assignment, gating, `Track.add_detection`, new tracks, `_clear_old_tracks` and the
`get_tracked_objects` selection.  Fed from `Regressor.regress` through `process_device` nothing leaves the device and
nothing synchronises until the tracked objects are read.

Deviations from the reference:
  * `rect` of a `TrackedObj` has 4 entries (left, top, right, bottom); the reference drags the detection's confidence and
    label through the box filter as truncated ints (6 entries), the demo reads `rect[:4]`;
  * no histories: only the last box / keypoints and the length of a track are kept, so `get_tracks()` and
    `get_archived_tracks()` raise;
  * the table is bounded: with `max_tracks` live tracks a detection that would open another one is not tracked and
    `dropped` counts it (the reference's list grows without bound);
  * keypoints are float64 throughout (the reference computes a new track's first update and interpolated entries in
    float32: a few 2^-24 on O(1) values).
"""
from collections import namedtuple

import numpy as np
import torch

from .. import _native as N

__all__ = ['IOUTracker', 'TrackedObj']

TrackedObj = namedtuple('TrackedObj', 'rect kp label')
LDS_PER_WORKGROUP = 160 * 1024       # gfx950
_UPLOADS_IN_FLIGHT = 4


class IOUTracker:
    """The reference's constructor arguments and defaults, then: `device`, `streams` (independent trackers -- cameras --
    advanced by one launch; the reference API addresses stream 0 and needs streams == 1), `max_detections` (per frame and
    stream) and `max_tracks` (live tracks per stream)."""

    def __init__(self,
                 time_window=5,
                 continue_time_thresh=2,
                 track_clear_thresh=3000,
                 match_threshold=0.4,
                 track_detection_iou_thresh=0.5,
                 interpolate_time_thresh=10,
                 detection_filter_speed=0.7,
                 keypoints_filter_speed=0.3,
                 add_treshold=0.1,
                 no_updated_frames_treshold=5,
                 align_kp=False,
                 device='cuda',
                 streams=1,
                 max_detections=64,
                 max_tracks=128):
        assert time_window >= 1
        self.time_window = time_window
        assert continue_time_thresh >= 1
        self.continue_time_thresh = continue_time_thresh
        assert track_clear_thresh >= 1
        self.track_clear_thresh = track_clear_thresh
        assert 0 <= match_threshold <= 1
        self.match_threshold = match_threshold
        assert 0 <= track_detection_iou_thresh <= 1
        self.track_detection_iou_thresh = track_detection_iou_thresh
        assert interpolate_time_thresh >= 0
        self.interpolate_time_thresh = interpolate_time_thresh
        assert 0 <= detection_filter_speed <= 1
        self.detection_filter_speed = detection_filter_speed
        assert 0 <= keypoints_filter_speed <= 1
        self.keypoints_filter_speed = keypoints_filter_speed
        assert 0 <= add_treshold <= 1
        self.add_treshold = add_treshold
        assert no_updated_frames_treshold >= 0
        assert isinstance(no_updated_frames_treshold, int)
        self.no_updated_frames_treshold = no_updated_frames_treshold
        self.align_kp = align_kp
        S, D, T = int(streams), int(max_detections), int(max_tracks)
        if S < 1 or D < 1 or T < 1:
            raise ValueError('streams, max_detections and max_tracks must be positive')
        self.streams, self.max_detections, self.max_tracks = S, D, T
        # the capacities are checked before anything touches the device: the kernel keeps the [D][T] cost matrix and the
        # assignment's working set in LDS
        lds = self.lds_bytes(D, T)
        if lds > LDS_PER_WORKGROUP:
            raise ValueError(f'max_detections={D} x max_tracks={T} needs {lds} bytes of LDS per workgroup, '
                             f'the device has {LDS_PER_WORKGROUP}')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('the tracker runs on the GPU (no CPU fallback)')
        self._state = None           # device buffers: allocated by the first call that needs them
        # outputs: one block, so that get_tracked_objects is one copy
        sizes = [('count', (S,), torch.int32), ('scalars', (S, 4), torch.int32), ('ids', (S, T), torch.int32),
                 ('boxes', (S, T, 4), torch.int32), ('kp', (S, T, 18), torch.float64)]
        self._out_layout, off = [], 0
        for name, shape, dt in sizes:
            nb = int(np.prod(shape)) * (8 if dt == torch.float64 else 4)
            self._out_layout.append((name, shape, dt, off, nb))
            off += (nb + 15) // 16 * 16
        self._out_bytes = off
        # host API: count + rects + keypoints of a frame in one pinned block; a few blocks, each with the event of its
        # last upload, so that filling the next frame does not wait for the previous copy
        self._in_layout = [('count', (1,), torch.int32, 0, 4), ('rects', (D, 4), torch.int32, 16, D * 16),
                           ('kp', (D, 18), torch.float32, 16 + D * 16, D * 72)]
        self._in_bytes = 16 + D * 88
        self._in_host, self._in_next = [], 0

    def _ensure(self):
        if self._state is None:
            sb = N.lib().t3d_track_state_bytes(self.max_tracks)
            if sb <= 0:
                raise RuntimeError(f't3d_track_state_bytes failed with code {sb}')
            self._state = torch.zeros(self.streams, sb, dtype=torch.uint8, device=self.device)   # all zero = a fresh tracker
            self._out = torch.zeros(self._out_bytes, dtype=torch.uint8, device=self.device)
            self._out_host = torch.zeros(self._out_bytes, dtype=torch.uint8).pin_memory()
            self._o, self._oh = self._views(self._out), self._views(self._out_host)
            self._in_block = torch.zeros(self._in_bytes, dtype=torch.uint8, device=self.device)
            self._in_dev = self._views(self._in_block, self._in_layout)

    @staticmethod
    def lds_bytes(max_detections, max_tracks):
        """LDS per workgroup of `t3d_track_step` at these capacities (a host-side query of the library)."""
        return N.lib().t3d_track_lds_bytes(int(max_detections), int(max_tracks))

    def _views(self, block, layout=None):
        return {name: block[off:off + nb].view(dt).view(shape) for name, shape, dt, off, nb in (layout or self._out_layout)}

    # ---- device API: no host synchronisation ---------------------------------------------------------------------------
    def process_batch_device(self, rects, kps, counts=None):
        """One frame of every stream: rects [S,D',4] int32, kps [S,D',18] float32 (D' <= max_detections), counts [S] int32
        (None: D' detections in every stream) -- device tensors; enqueues one launch."""
        S, T = self.streams, self.max_tracks
        if rects.dim() != 3 or rects.shape[0] != S or rects.shape[2] != 4:
            raise ValueError(f'rects must be [{S}, n, 4]')
        D = int(rects.shape[1])
        if D > self.max_detections:
            raise ValueError(f'{D} detections per stream, the tracker was built for max_detections={self.max_detections}')
        kps = kps.reshape(S, D, 18)
        assert rects.dtype == torch.int32 and kps.dtype == torch.float32, 'rects int32, keypoints float32'
        assert counts is None or (counts.dtype == torch.int32 and counts.numel() == S)
        for t in (rects, kps, counts):
            assert t is None or (t.is_cuda and t.is_contiguous()), 'the device API takes contiguous device tensors'
        self._ensure()
        o = self._o
        N.call('t3d_track_step', N.ptr(self._state), N.ptr(rects) if D else None, N.ptr(kps) if D else None,
               N.ptr(counts), S, D, T, int(self.time_window), int(self.continue_time_thresh), int(self.track_clear_thresh),
               float(self.match_threshold), float(self.track_detection_iou_thresh), int(self.interpolate_time_thresh),
               float(self.detection_filter_speed), float(self.keypoints_filter_speed), float(self.add_treshold),
               int(self.no_updated_frames_treshold), int(bool(self.align_kp)), N.ptr(o['count']), N.ptr(o['boxes']),
               N.ptr(o['kp']), N.ptr(o['ids']), N.ptr(o['scalars']), N.stream())

    def process_device(self, rects, kps, counts=None):
        """One frame of a single-stream tracker from what `Regressor.regress` has on the device: rects [n,4] int32 and
        kp [n,9,2] (or [n,18]) float32; counts: [1] int32 device tensor when fewer than n rows are valid."""
        if self.streams != 1:
            raise ValueError('process_device addresses a single-stream tracker; use process_batch_device')
        n = int(rects.shape[0])
        self.process_batch_device(rects.reshape(1, n, 4), kps.reshape(1, n, 18), counts)

    def tracked_device(self):
        """The last frame's outputs as device tensors (views into the tracker's buffers, overwritten by the next frame):
        dict(count [S], boxes [S,T,4] int32, kp [S,T,18] float64, ids [S,T] int32 with -1 for tracks not longer than
        time_window, scalars [S,4] = num_tracks, last_global_id, time, dropped); rows past `count` are stale."""
        self._ensure()
        return dict(self._o)

    # ---- the reference's host API ------------------------------------------------------------------------------------------
    def process(self, frame, detections, kps):
        """`detections`: the detector's (left, top, right, bottom, confidence, label) tuples, `kps`: one 18-vector each;
        `frame` is not looked at (as in the reference).  One pinned upload, one launch, no synchronisation."""
        if self.streams != 1:
            raise ValueError('process addresses a single-stream tracker; use process_batch_device')
        n = len(detections)
        if n > self.max_detections:
            raise ValueError(f'{n} detections, the tracker was built for max_detections={self.max_detections}')
        assert len(kps) == n
        self._ensure()
        if len(self._in_host) < _UPLOADS_IN_FLIGHT:
            block = torch.zeros(self._in_bytes, dtype=torch.uint8).pin_memory()
            self._in_host.append((block, self._views(block, self._in_layout), torch.cuda.Event()))
        block, host, done = self._in_host[self._in_next]
        self._in_next = (self._in_next + 1) % _UPLOADS_IN_FLIGHT
        done.synchronize()            # (the copy that last read this block, several frames ago: returns at once)
        host['count'][0] = n
        if n:
            host['rects'][:n] = torch.as_tensor([[int(v) for v in d[:4]] for d in detections], dtype=torch.int32)
            host['kp'][:n] = torch.as_tensor(np.asarray(kps, dtype=np.float32).reshape(n, 18))
        dev = self._in_dev
        self._in_block.copy_(block, non_blocking=True)
        done.record()
        self.process_batch_device(dev['rects'].view(1, -1, 4), dev['kp'].view(1, -1, 18), dev['count'])

    def get_tracked_objects(self):
        """[TrackedObj(rect, kp, label)] of the tracks the last frame touched, in track-list order: rect a 4-tuple of ints,
        kp a tuple of 18 floats, label 'ID n' or 'ID -1' (track not longer than time_window).  The one call that waits for
        the device."""
        if self.streams != 1:
            raise ValueError('get_tracked_objects addresses a single-stream tracker; read tracked_device()')
        self._ensure()
        self._out_host.copy_(self._out, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        h = self._oh
        n = int(h['count'][0])
        boxes, kp, ids = h['boxes'][0, :n].tolist(), h['kp'][0, :n].tolist(), h['ids'][0, :n].tolist()
        return [TrackedObj(tuple(boxes[i]), tuple(kp[i]), f'ID {ids[i]}') for i in range(n)]

    def _scalar(self, k):
        self._ensure()
        v = self._o['scalars'][:, k].cpu().tolist()
        return v[0] if self.streams == 1 else v

    @property
    def num_tracks(self):
        """Live tracks (`len(tracker.tracks)` in the reference); a list with streams > 1.  Synchronises."""
        return self._scalar(0)

    @property
    def last_global_id(self):
        return self._scalar(1)

    @property
    def time(self):
        return self._scalar(2)

    @property
    def dropped(self):
        """Detections that found the table of `max_tracks` tracks full and were not tracked."""
        return self._scalar(3)

    def get_tracks(self):
        raise NotImplementedError('track histories are not kept on the device: only the last box / keypoints and the length '
                                  'of each track live in the state block; read get_tracked_objects() or tracked_device()')

    def get_archived_tracks(self):
        raise NotImplementedError('track histories are not kept on the device: tracks that leave through track_clear_thresh '
                                  'are counted, not archived')
