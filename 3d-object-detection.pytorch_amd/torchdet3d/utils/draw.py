"""The last stage of the live loop on the HIP path: boxes, keypoints and labels drawn on frames on the device.

Mirrors `draw_detections` (scripts/demo.py:26-46) and `draw_kp` (torchdet3d/utils/utils.py:247-270) of the reference: one launch
of `t3d_draw_overlays_u8` (csrc/draw.hip) draws, for every camera and tracked object, the detector's rectangle, the 12 box
edges, the 9 keypoints and a label plate with the class name -- in place, without a read-back or a synchronisation.

Deviations from the reference:
  * OpenCV and objectron.graphics are not available, so the raster rules are this project's own (integer arithmetic, stated
    in DESIGN.md section 7) and the LOOK -- colours, thickness, the 5 x 7 font -- is unpinned against the reference's output;
  * `draw_kp` returns the annotated copy in the INPUT's channel order (the reference hands back BGR for `cv.imwrite`; here
    Pillow writes the file and wants RGB), always HWC, and puts the label on a plate in the top-left corner (the reference
    writes it at (10, 180));
  * there is no CPU fallback: drawing needs the GPU.
"""
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native as N
from .utils import OBJECTRON_CLASSES

__all__ = ['DrawStyle', 'draw_overlays', 'draw_kp']


@dataclass
class DrawStyle:
    """Thickness, sizes and colours of the overlays.  Colours are written as (R, G, B); `bgr=True` is for frames in OpenCV's
    channel order: every colour is packed reversed.  `draw_ids` appends the track id to the class name."""
    rect_th: int = 2
    edge_th: int = 2
    kp_radius: int = 3
    font_scale: int = 2
    draw_ids: bool = False
    bgr: bool = False
    rect: tuple = (0, 255, 0)                 # scripts/demo.py:35
    rect_off: tuple = (100, 100, 100)         # scripts/demo.py:37: a track not longer than time_window ('ID -1')
    edge_x: tuple = (255, 0, 0)
    edge_y: tuple = (0, 255, 0)
    edge_z: tuple = (0, 0, 255)
    keypoint: tuple = (255, 255, 0)
    plate: tuple = (255, 255, 255)            # scripts/demo.py:42-44
    text: tuple = (0, 0, 0)

    def pack(self):
        """-> the `t3d_draw_style` the launch copies (include/t3d.h)."""
        for name, lo, hi in (('rect_th', 1, 16), ('edge_th', 1, 16), ('kp_radius', 0, 32), ('font_scale', 1, 8)):
            v = getattr(self, name)
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= v <= hi:
                raise ValueError(f'{name} must be an integer in {lo}..{hi}, not {v!r}')
        st = N.DrawStyleC(int(self.rect_th), int(self.edge_th), int(self.kp_radius), int(self.font_scale),
                          N.DRAW_IDS if self.draw_ids else 0)
        for i, name in enumerate(('rect', 'rect_off', 'edge_x', 'edge_y', 'edge_z', 'keypoint', 'plate', 'text')):
            c = tuple(getattr(self, name))
            if len(c) != 3 or any(not isinstance(v, (int, np.integer)) or not 0 <= v <= 255 for v in c):
                raise ValueError(f'{name} must be three integers in 0..255, not {c!r}')
            for j, v in enumerate(reversed(c) if self.bgr else c):
                st.colors[i][j] = int(v)
        return st


def _i32(t, shape, what, device):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape):
        raise ValueError(f'{what} must be a contiguous int32 device tensor {list(shape)}')
    if t.device != device:
        raise ValueError(f'{what} on {t.device}, the frames on {device}')
    return t


def draw_overlays(frames, kp, boxes=None, ids=None, labels=None, count=None, label_count=None, style=None):
    """Draws on `frames` (uint8 device tensor [S,H,W,3], or [H,W,3] for one camera; contiguous) IN PLACE and returns it.

    kp [S,T,18] (or [S,T,9,2]) float64 keypoints in frame pixels; boxes [S,T,4] int32 (left, top, right, bottom) or None: no
    rectangles, plates in the top-left corner; ids [S,T] int32 or None (ids < 0: grey rectangle, no keypoints); labels
    [S,L] int32 class indices or None, object t takes labels[s, t] when t < label_count[s] (None: every entry, L >= T);
    count [S] int32 objects per camera or None: T.  `style`: a `DrawStyle` (or its packed form).  One launch on the current
    stream; never synchronises."""
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8):
        raise ValueError('frames must be a uint8 device tensor')
    f4 = frames.unsqueeze(0) if frames.dim() == 3 else frames
    if f4.dim() != 4 or f4.shape[3] != 3:
        raise ValueError('frames must be [S, H, W, 3] (or [H, W, 3])')
    if not f4.is_contiguous():
        raise ValueError('frames must be contiguous: the overlays are drawn in place')
    S, H, W = (int(v) for v in f4.shape[:3])
    if not (torch.is_tensor(kp) and kp.is_cuda and kp.dtype == torch.float64 and kp.is_contiguous()):
        raise ValueError('kp must be a contiguous float64 device tensor')
    if kp.dim() < 3 or kp.shape[0] != S or kp.numel() != S * int(kp.shape[1]) * 18 or kp.device != f4.device:
        raise ValueError(f'kp must be [{S}, T, 18] on the frames\' device')
    T = int(kp.shape[1])
    dev = f4.device
    boxes, ids = _i32(boxes, (S, T, 4), 'boxes', dev), _i32(ids, (S, T), 'ids', dev)
    count, label_count = _i32(count, (S,), 'count', dev), _i32(label_count, (S,), 'label_count', dev)
    stride = 0
    if labels is not None:
        if labels.dim() != 2:
            raise ValueError(f'labels must be [{S}, L]')
        stride = int(labels.shape[1])
        labels = _i32(labels, (S, stride), 'labels', dev)
    if style is None:
        style = DrawStyle()
    st = style.pack() if isinstance(style, DrawStyle) else style
    N.call('t3d_draw_overlays_u8', N.ptr(f4), S, H, W, N.ptr(count), N.ptr(boxes), N.ptr(kp), N.ptr(ids), N.ptr(labels),
           N.ptr(label_count), stride, T, st, N.stream())
    return frames


def _label_index(label):
    if label is None:
        return None
    if isinstance(label, str):
        if label not in OBJECTRON_CLASSES:
            raise ValueError(f'label {label!r} is not one of {OBJECTRON_CLASSES}')
        return OBJECTRON_CLASSES.index(label)
    if isinstance(label, (int, np.integer)) and not isinstance(label, bool) and 0 <= label < len(OBJECTRON_CLASSES):
        return int(label)
    raise ValueError(f'label must be a class name or an index in 0..{len(OBJECTRON_CLASSES) - 1}, not {label!r}')


def draw_kp(img, keypoints, name=None, normalized=True, RGB=True, num_keypoints=9, label=None, style=None, device='cuda'):
    """The reference's `draw_kp` (utils/utils.py:247-270): img uint8 [H,W,3] or [3,H,W] (numpy or tensor), keypoints [9,2]
    normalised to the image (`normalized=True`: multiplied by (w, h) in float64) or in pixels, label a class name or index.
    Returns an annotated numpy COPY [H,W,3] in the input's channel order (`RGB=False`: the colours are packed for BGR);
    `name`: also saved there through Pillow.  Waits for the device (a host API)."""
    if num_keypoints != 9:
        raise ValueError(f'num_keypoints must be 9 (the box centre and its 8 vertices), not {num_keypoints}')
    lab = _label_index(label)
    arr = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if arr.dtype != np.uint8 or arr.ndim != 3:
        raise ValueError('img must be uint8 with three dimensions')
    if arr.shape[0] == 3:                          # utils.py:255-256: a transposed image
        arr = np.transpose(arr, (1, 2, 0))
    if arr.shape[2] != 3:
        raise ValueError('img must be [H, W, 3] or [3, H, W]')
    kp = np.array(keypoints.detach().cpu().numpy() if torch.is_tensor(keypoints) else keypoints, np.float64)
    if kp.size != 18:
        raise ValueError('keypoints must be [9, 2]')
    kp = kp.reshape(9, 2)
    h, w = arr.shape[:2]
    if normalized:
        kp = kp * np.asarray([w, h], np.float64)
    if not torch.cuda.is_available():
        raise RuntimeError('drawing runs on the GPU (no CPU fallback)')
    if style is None:
        style = DrawStyle(bgr=not RGB)
    frame = torch.from_numpy(np.ascontiguousarray(arr)).to(device).unsqueeze(0)
    kd = torch.from_numpy(kp.reshape(1, 1, 18)).to(device)
    labels = None if lab is None else torch.tensor([[lab]], dtype=torch.int32, device=device)
    out = draw_overlays(frame, kd, labels=labels, style=style)[0].cpu().numpy()
    if name:
        from PIL import Image
        Image.fromarray(out if RGB else np.ascontiguousarray(out[:, :, ::-1])).save(name)
    return out
