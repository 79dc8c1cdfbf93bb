"""The detector's dataset and its training pipeline (configs/detection/mnv2_ssd_300_2_heads.py:63-143), pixel work on the GPU.

`ObjectronFrames` is the host half: one item per IMAGE of the COCO-style json `Objectron` reads one item per annotation
from -- the decoded frame, its boxes and labels -- with the filters of mmdet's published `CocoDataset`.  It runs in
DataLoader workers and draws nothing.

`DetectionAugmentPipeline` compiles the config's mmdet-style `train_pipeline` / `test_pipeline` (lists of dicts) into the
per-sample random draws, the box arithmetic (host, float32) and the `t3d_det_sample` records of one `t3d_detect_augment_u8`
launch per batch (csrc/detect_augment.hip, driven by dataloaders/gpu_detection_loader.py).  Any transform type or setting
that is not built raises NotImplementedError naming it.

The transforms are those of the PUBLISHED mmdet 2.x sources (PhotoMetricDistortion, Expand, MinIoURandomCrop, Resize,
RandomFlip; `RandomRotate90and270` is the fork's albumentations add-on: a quarter turn k in {1, 3} in np.rot90's sense), recalled,
not linked.  The fork that ran the config is external, so parity with it is UNPINNED: include/t3d.h, this file and the numpy
restatement tests/detect_augment_ref.py are the definition.  The JPEG decoder is Pillow (cv2.imread in mmdet): UNPINNED too.
mmdet draws inside its workers with `random` / `np.random`; here every draw happens in the main process from numpy
Generators keyed (seed, epoch, rank, batch), so batches are reproducible and do not depend on the number of workers, and the
reference's random stream is not reproduced.

Deviation: mmdet hands the network the unclipped float32 image / 255 (`Normalize` with mean 0, std 255 -- the stem applies
it here, so the step compiles to nothing); the kernel rounds (half to even) and saturates to uint8 once at the end.
"""
import itertools
import json
import os
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from ..utils import OBJECTRON_CLASSES

__all__ = ['ObjectronFrames', 'DetectionAugmentPipeline', 'collate_frames', 'resize_boxes', 'DET_SAMPLE_DTYPE']

# include/t3d.h: t3d_det_sample (80 bytes) and its flags
DET_SAMPLE_DTYPE = np.dtype([('offset', '<i8'), ('h', '<i4'), ('w', '<i4'), ('turns', '<i4'), ('left', '<i4'), ('top', '<i4'),
                             ('cx0', '<i4'), ('cy0', '<i4'), ('cx1', '<i4'), ('cy1', '<i4'), ('flags', '<i4'), ('delta', '<f4'),
                             ('alpha', '<f4'), ('sat', '<f4'), ('hue', '<f4'), ('perm', '<i4', (3,)), ('reserved', '<i4')])
assert DET_SAMPLE_DTYPE.itemsize == 80
DET_FLIP, DET_BRIGHTNESS, DET_CONTRAST, DET_CONTRAST_LAST, DET_HSV, DET_SATURATION, DET_HUE = 1, 2, 4, 8, 16, 32, 64
# the crop search of sample i draws from its own Generator keyed (*key, _CROP_TAG, i): its length depends on the boxes
_CROP_TAG = 0x5D3C0A7E11F2
_PERMS = np.array(list(itertools.permutations(range(3))), np.int32)


class ObjectronFrames(torch.utils.data.Dataset):
    """One item per image: (frame uint8 [h, w, 3] RGB decoded with Pillow, boxes float32 [n, 4] = (x, y, x + w, y + h) of
    'bbox', labels int32 [n] = category_id - 1).

    root: the folder the json's file names are relative to, with `annotations/objectron_{train,test}.json` (mode 'train' /
    'val' or 'test') -- or pass `ann_file` to name the json itself.  Filters, as mmdet's CocoDataset: an annotation is dropped
    when it is `iscrowd`, when its w < 1 or h < 1, or when its category is outside `category_list` (names of
    OBJECTRON_CLASSES; 'all' keeps every one; the label stays category_id - 1, it is not renumbered); in train mode an image
    is dropped when no box is left or when min(width, height) < min_size.
    Index: the images that survive, in the order of the json's 'images' list -- dataset index i is the i-th of them, whatever
    their ids are; `image_ids[i]` is its id.

    decode='device' (dataloaders/jpeg.py): after `build_index()` an item is (the FILE's bytes uint8 [n], boxes, labels, i) and
    the frame is decoded on the device by `GpuDetectionLoader`; for a file the index keeps on the host (progressive, restart
    markers, 4:2:2, not a JPEG, ...) the payload is the host-decoded frame [h, w, 3] instead.  The workers then only read
    files; they never touch the native library."""

    def __init__(self, root, mode='train', category_list='all', min_size=17, ann_file=None, decode='host'):
        if mode not in ('train', 'val', 'test'):
            raise RuntimeError('Unknown dataset mode')
        if decode not in ('host', 'device'):
            raise ValueError(f"decode={decode!r}: 'host' or 'device'")
        self.root, self.mode, self.decode, self.index = str(root), mode, decode, None
        if ann_file is None:
            ann_file = Path(root).resolve() / ('annotations/objectron_train.json' if mode == 'train'
                                               else 'annotations/objectron_test.json')
        with open(ann_file, 'r') as f:
            ann = json.load(f)
        keep_cat = None if category_list == 'all' else set(category_list)
        per_image = {}
        for a in ann['annotations']:
            x, y, w, h = (float(v) for v in a['bbox'])
            if a.get('iscrowd', 0) or w < 1 or h < 1:
                continue
            cat = int(a['category_id']) - 1
            if keep_cat is not None and not (0 <= cat < len(OBJECTRON_CLASSES) and OBJECTRON_CLASSES[cat] in keep_cat):
                continue
            per_image.setdefault(a['image_id'], []).append((x, y, x + w, y + h, cat))
        self.files, self.image_ids, self._boxes, self._labels = [], [], [], []
        for img in ann['images']:
            rows = per_image.get(img['id'], [])
            if mode == 'train':
                if not rows:
                    continue
                if 'width' in img and 'height' in img:
                    wh = int(img['width']), int(img['height'])
                else:
                    with Image.open(self.root + '/' + img['file_name']) as im:
                        wh = im.size
                if min(wh) < min_size:
                    continue
            self.files.append(img['file_name'])
            self.image_ids.append(img['id'])
            arr = np.asarray(rows, np.float64).reshape(-1, 5)
            self._boxes.append(arr[:, :4].astype(np.float32))
            self._labels.append(arr[:, 4].astype(np.int32))

    def __len__(self):
        return len(self.files)

    def build_index(self, path=None, threads=8, seg_mcus=None):
        """The JPEG index `decode='device'` needs, like `fill_cache()` on the regression side: loaded from `path` when that file
        exists (memory-mapped; every file's size and mtime are checked against it and a changed file raises, naming it), else
        built with `threads` host threads of this process and, with a `path`, saved there.  -> the `JpegIndex`."""
        from .jpeg import DEFAULT_SEG_MCUS, JpegIndex
        if path is not None and os.path.exists(path):
            index = JpegIndex.load(path, mmap_mode='r' if not str(path).endswith('.npz') else None)
            if index.files != self.files:
                raise RuntimeError(f'{path} indexes other files than this dataset holds: rebuild the index')
            if seg_mcus is not None and index.seg_mcus != int(seg_mcus):
                raise RuntimeError(f'{path} was built with seg_mcus = {index.seg_mcus}, not {seg_mcus}: rebuild the index')
            index.check(self.root)
        else:
            index = JpegIndex.build(self.files, self.root, seg_mcus or DEFAULT_SEG_MCUS, threads)
            if path is not None:
                index.save(path)
        self.index = index
        return index

    def _decode_host(self, path):
        with Image.open(path) as im:
            return np.asarray(im.convert('RGB'))

    def __getitem__(self, i):
        path = self.root + '/' + self.files[i]
        if self.decode == 'host':
            return self._decode_host(path), self._boxes[i].copy(), self._labels[i].copy()
        if self.index is None:
            raise RuntimeError("ObjectronFrames(decode='device'): call build_index() first")
        if int(self.index.reason[i]) != 0:
            payload = self._decode_host(path)
        else:
            payload = np.fromfile(path, np.uint8)
            if payload.size != int(self.index.size[i]):
                raise RuntimeError(f'{path} changed since it was indexed ({payload.size} bytes now, {int(self.index.size[i])} in '
                                   f'the index): rebuild the index')
        return payload, self._boxes[i].copy(), self._labels[i].copy(), i


def collate_frames(items):
    """DataLoader collate: frames of any size packed into one uint8 buffer with a descriptor table.
    -> (packed uint8 [bytes], desc int64 [B, 3] = (offset, h, w), boxes float32 [sum n, 4], labels int32 [sum n],
    counts int64 [B])."""
    desc = np.zeros((len(items), 3), np.int64)
    off = 0
    for i, (f, _, _) in enumerate(items):
        desc[i] = off, f.shape[0], f.shape[1]
        off += f.shape[0] * f.shape[1] * 3
    packed = np.empty(max(off, 1), np.uint8)
    for (f, _, _), (o, h, w) in zip(items, desc):
        packed[o:o + h * w * 3].reshape(h, w, 3)[...] = f
    boxes = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for _, b, _ in items])
    labels = np.concatenate([np.asarray(l, np.int32).reshape(-1) for _, _, l in items])
    counts = np.asarray([len(l) for _, _, l in items], np.int64)
    return (torch.from_numpy(packed), torch.from_numpy(desc), torch.from_numpy(boxes), torch.from_numpy(labels),
            torch.from_numpy(counts))


def resize_boxes(boxes, row, h, w, size):
    """mmdet's Resize of the boxes of a batch, scale then clip to the image: boxes float32 [n, 4], row [n] the image each
    belongs to, h and w int64 [B] of the frames, size (oh, ow) of the output.  -> float32 [n, 4]."""
    oh, ow = size
    sc = np.stack([ow / w, oh / h, ow / w, oh / h], 1).astype(np.float32)
    return np.minimum(np.maximum(boxes * sc[row], np.float32(0)), np.array([ow, oh, ow, oh], np.float32))


# the order the kernel applies the steps in: the config's
_ORDER = ('PhotoMetricDistortion', 'Albu', 'Expand', 'MinIoURandomCrop', 'Resize', 'RandomFlip')
_SETTINGS = {
    'LoadImageFromFile': ('to_float32',),
    'LoadAnnotations': ('with_bbox',),
    'PhotoMetricDistortion': ('brightness_delta', 'contrast_range', 'saturation_range', 'hue_delta'),
    'Albu': ('transforms', 'bbox_params', 'update_pad_shape', 'skip_img_without_anno'),
    'Expand': ('mean', 'to_rgb', 'ratio_range', 'prob'),
    'MinIoURandomCrop': ('min_ious', 'min_crop_size', 'bbox_clip_border'),
    'Resize': ('img_scale', 'keep_ratio'),
    'Normalize': ('mean', 'std', 'to_rgb'),
    'RandomFlip': ('flip_ratio', 'direction'),
    'DefaultFormatBundle': (),
    'Collect': ('keys', 'meta_keys'),
    'MultiScaleFlipAug': ('img_scale', 'flip', 'transforms'),
    'ImageToTensor': ('keys',),
}


def _refuse(what):
    raise NotImplementedError(f'{what} is not built for the GPU detection pipeline (built: {", ".join(_SETTINGS)})')


class DetectionAugmentPipeline:
    """A compiled mmdet-style pipeline: `size` (oh, ow), the per-sample draws, the box arithmetic and the kernel records.

    draw(n, key) -> the parameters of n samples; boxes(boxes, labels, desc, prm) -> the transformed boxes and labels -- it also
    runs MinIoURandomCrop's search, which needs the boxes, and leaves the geometry it chose in prm['geom'];
    records(desc, prm) -> [n] t3d_det_sample, after boxes().  `random`: some step draws (a training pipeline); a pipeline that
    is `Resize` alone is the test path, which the loader runs through t3d_augment_crops_u8."""

    def __init__(self, steps, size=(300, 300)):
        self.size = (int(size[0]), int(size[1]))
        self.photo = self.p_rot = self.expand = self.crop = None
        self.p_flip = 0.0
        self.has_resize = False
        seen = []
        self._compile(steps, seen)
        geo = [t for t in seen if t in _ORDER]
        for t in set(geo):
            if geo.count(t) > 1:
                _refuse(f'{t} appearing {geo.count(t)} times')
        if geo != [t for t in _ORDER if t in geo]:
            _refuse(f'the order {" -> ".join(geo)} (the kernel applies {" -> ".join(_ORDER)})')
        if not self.has_resize:
            raise ValueError('the pipeline needs a Resize: frames of different sizes cannot be batched')

    def _compile(self, steps, seen):
        oh, ow = self.size
        for step in steps:
            a = dict(step)
            t = a.pop('type', None)
            if t not in _SETTINGS:
                _refuse(f'transform {t!r}')
            for k in a:
                if k not in _SETTINGS[t]:
                    _refuse(f'{t}: setting {k!r}')
            seen.append(t)
            if t == 'LoadAnnotations':
                if not a.get('with_bbox', True):
                    _refuse('LoadAnnotations: with_bbox=False')
            elif t in ('Collect', 'ImageToTensor'):
                allowed = ('img', 'gt_bboxes', 'gt_labels') if t == 'Collect' else ('img',)
                for k in a.get('keys', ()):
                    if k not in allowed:
                        _refuse(f'{t}: key {k!r} (the loader yields {", ".join(allowed)})')
            elif t == 'PhotoMetricDistortion':
                clo, chi = a.get('contrast_range', (0.5, 1.5))
                slo, shi = a.get('saturation_range', (0.5, 1.5))
                self.photo = dict(delta=float(a.get('brightness_delta', 32)), contrast=(float(clo), float(chi)),
                                  saturation=(float(slo), float(shi)), hue=float(a.get('hue_delta', 18)))
            elif t == 'Albu':
                # the boxes turn with the frame and none is lost by a quarter turn: only settings that say the same pass
                bp = dict(a.get('bbox_params') or {})
                for k, v in bp.items():
                    if k not in ('type', 'format', 'label_fields', 'min_visibility', 'min_area', 'filter_lost_elements') \
                            or (k == 'type' and v != 'BboxParams') or (k == 'format' and v != 'pascal_voc') \
                            or (k in ('min_visibility', 'min_area') and v != 0) \
                            or (k == 'label_fields' and list(v) != ['gt_labels']):
                        _refuse(f'Albu: bbox_params {k}={v!r}')
                if a.get('update_pad_shape', False):
                    _refuse('Albu: update_pad_shape=True')
                for sub in a.get('transforms', ()):
                    sub = dict(sub)
                    st = sub.pop('type', None)
                    if st != 'RandomRotate90and270':
                        _refuse(f'Albu: transform {st!r}')
                    for k in sub:
                        if k not in ('p', 'always_apply'):
                            _refuse(f'Albu: RandomRotate90and270: setting {k!r}')
                    if self.p_rot is not None:
                        _refuse('Albu: RandomRotate90and270 appearing twice')
                    self.p_rot = 1.0 if sub.get('always_apply', False) else self._number('Albu: RandomRotate90and270', 'p', sub.get('p', 0.5))
            elif t == 'Expand':
                if any(float(v) != 0 for v in a.get('mean', (0, 0, 0))):
                    _refuse(f'Expand: mean={a["mean"]!r} (only a fill of 0)')
                lo, hi = a.get('ratio_range', (1, 4))
                if not 1 <= lo <= hi:
                    raise ValueError(f'Expand: ratio_range={(lo, hi)!r}')
                # (to_rgb only reorders `mean`, which is 0)
                self.expand = dict(ratio=(float(lo), float(hi)), p=self._number('Expand', 'prob', a.get('prob', 0.5)))
            elif t == 'MinIoURandomCrop':
                if not a.get('bbox_clip_border', True):
                    _refuse('MinIoURandomCrop: bbox_clip_border=False')
                self.crop = dict(modes=(1.0,) + tuple(float(v) for v in a.get('min_ious', (0.1, 0.3, 0.5, 0.7, 0.9))) + (0.0,),
                                 min_size=float(a.get('min_crop_size', 0.3)))
            elif t in ('Resize', 'MultiScaleFlipAug'):
                if t == 'Resize' and a.get('keep_ratio', True):
                    _refuse('Resize: keep_ratio=True')
                if t == 'MultiScaleFlipAug' and a.get('flip', False):
                    _refuse('MultiScaleFlipAug: flip=True')
                if 'img_scale' in a:
                    sc = a['img_scale']
                    if isinstance(sc, list) or len(sc) != 2 or (int(sc[0]), int(sc[1])) != (ow, oh):
                        _refuse(f'{t}: img_scale={sc!r} (only the one (w, h) = {(ow, oh)} of `size`)')
                if t == 'Resize':
                    self.has_resize = True
                else:
                    self._compile(a.get('transforms', ()), seen)
            elif t == 'Normalize':
                mean, std = a.get('mean', None), a.get('std', None)
                if mean is None or std is None or any(float(v) != 0 for v in mean) or any(float(v) != 255 for v in std):
                    _refuse(f'Normalize: mean={mean!r}, std={std!r} (only mean 0 / std 255, which the stem applies)')
            elif t == 'RandomFlip':
                if a.get('direction', 'horizontal') != 'horizontal':
                    _refuse(f'RandomFlip: direction={a["direction"]!r}')
                self.p_flip = self._number('RandomFlip', 'flip_ratio', a.get('flip_ratio') or 0.0)

    @staticmethod
    def _number(t, k, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            _refuse(f'{t}: {k}={v!r} (one number)')
        return float(v)

    @property
    def random(self):
        return bool(self.photo or self.p_rot or self.expand or self.crop or self.p_flip)

    def draw(self, n, key):
        """Per-sample parameters from numpy Generator(key), key = (seed, epoch, rank, batch[, item]): `random((n, 18))`,
        columns  0 brightness fires (u < .5)  1 delta   2 contrast fires  3 alpha  4 contrast in front of the HSV block (u < .5)
          5 saturation fires  6 factor   7 hue fires  8 shift   9 permutation fires  10 floor(6 u) indexes
          itertools.permutations(range(3))   11 quarter turn fires  12 k = 1 (u < .5) or 3   13 expand fires  14 ratio
          15, 16 paste position   17 flip fires.
        -> dict: bright, contrast, first, sat_on, hue_on, turn, expand, flip (bool), delta, alpha, sat, hue (float32), perm
        (int32 [n, 3]), turns (int32: 0, 1, 3), ratio, u_left, u_top (float64), key (for the crop search's own Generators)."""
        u = np.random.default_rng([int(k) for k in key]).random((n, 18))
        ph = self.photo or dict(delta=0., contrast=(1., 1.), saturation=(1., 1.), hue=0.)
        on = self.photo is not None

        def lin(lo, hi, col):
            return (lo + (hi - lo) * u[:, col]).astype(np.float32)
        turn = u[:, 11] < (self.p_rot or 0.0)
        ex = self.expand or dict(ratio=(1., 1.), p=0.)
        return dict(bright=on & (u[:, 0] < .5), delta=lin(-ph['delta'], ph['delta'], 1), contrast=on & (u[:, 2] < .5),
                    alpha=lin(*ph['contrast'], 3), first=u[:, 4] < .5, sat_on=on & (u[:, 5] < .5), sat=lin(*ph['saturation'], 6),
                    hue_on=on & (u[:, 7] < .5), hue=lin(-ph['hue'], ph['hue'], 8),
                    perm=np.where((on & (u[:, 9] < .5))[:, None], _PERMS[np.minimum((u[:, 10] * 6).astype(np.int64), 5)],
                                  _PERMS[0][None]).astype(np.int32),
                    turn=turn, turns=np.where(turn, np.where(u[:, 12] < .5, 1, 3), 0).astype(np.int32),
                    expand=u[:, 13] < ex['p'], ratio=ex['ratio'][0] + (ex['ratio'][1] - ex['ratio'][0]) * u[:, 14],
                    u_left=u[:, 15], u_top=u[:, 16], flip=u[:, 17] < self.p_flip, key=[int(k) for k in key])

    def _min_iou_crop(self, b, h, w, rng):
        """mmdet's MinIoURandomCrop.__call__ on boxes b (float32 [n, 4]) in an h x w image -> (mode, patch or None, mask)."""
        modes, lo = self.crop['modes'], self.crop['min_size']
        while True:
            mode = modes[int(rng.random() * len(modes))]
            if mode == 1:
                return mode, None, np.ones(len(b), bool)
            for _ in range(50):
                new_w = lo * w + (w - lo * w) * rng.random()
                new_h = lo * h + (h - lo * h) * rng.random()
                if new_h / new_w < 0.5 or new_h / new_w > 2:
                    continue
                left, top = rng.random() * (w - new_w), rng.random() * (h - new_h)
                patch = np.array((int(left), int(top), int(left + new_w), int(top + new_h)), np.int64)
                if patch[2] == patch[0] or patch[3] == patch[1]:
                    continue
                pf = patch.astype(np.float32)
                if len(b):
                    iw = np.maximum(np.minimum(b[:, 2], pf[2]) - np.maximum(b[:, 0], pf[0]), np.float32(0))
                    ih = np.maximum(np.minimum(b[:, 3], pf[3]) - np.maximum(b[:, 1], pf[1]), np.float32(0))
                    inter = iw * ih
                    union = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) + (pf[2] - pf[0]) * (pf[3] - pf[1]) - inter
                    if (inter / np.maximum(union, np.float32(1e-6))).min() < mode:
                        continue
                    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
                    mask = (cx > pf[0]) & (cy > pf[1]) & (cx < pf[2]) & (cy < pf[3])
                    if not mask.any():
                        continue
                else:
                    mask = np.zeros(0, bool)
                return mode, patch, mask

    def boxes(self, boxes, labels, desc, prm):
        """boxes: per sample float32 [n_i, 4] in frame pixels, labels: per sample int32 [n_i], desc int64 [B, 3] (offset, h, w)
        -> (boxes, labels) per sample in output pixels, after every step (host, float32).  Leaves in prm: 'geom' int64 [B, 7]
        = (turns, left, top, cx0, cy0, cx1, cy1) for records(), 'canvas' int64 [B, 2] = (H, W), 'mode' float64 [B] (the crop
        mode that returned; 1 without a crop)."""
        oh, ow = self.size
        B = len(desc)
        geom, canvas, modes = np.zeros((B, 7), np.int64), np.zeros((B, 2), np.int64), np.ones(B, np.float64)
        out_b, out_l = [], []
        for i in range(B):
            b, l = np.array(boxes[i], np.float32).reshape(-1, 4), np.asarray(labels[i], np.int32).reshape(-1)
            h, w = int(desc[i, 1]), int(desc[i, 2])
            k = int(prm['turns'][i])
            if k == 1:                 # np.rot90(frame, 1): x' = y, y' = w - x
                b = np.stack([b[:, 1], np.float32(w) - b[:, 2], b[:, 3], np.float32(w) - b[:, 0]], 1)
                h, w = w, h
            elif k == 3:               # np.rot90(frame, 3): x' = h - y, y' = x
                b = np.stack([np.float32(h) - b[:, 3], b[:, 0], np.float32(h) - b[:, 1], b[:, 2]], 1)
                h, w = w, h
            left = top = 0
            if prm['expand'][i]:
                r = float(prm['ratio'][i])
                H, W = int(h * r), int(w * r)
                left, top = int(float(prm['u_left'][i]) * (W - w)), int(float(prm['u_top'][i]) * (H - h))
                b = b + np.array([left, top, left, top], np.float32)
                h, w = H, W
            canvas[i] = h, w
            patch = None
            if self.crop is not None:
                rng = np.random.default_rng(prm['key'] + [_CROP_TAG, i])
                modes[i], patch, mask = self._min_iou_crop(b, h, w, rng)
            if patch is None:
                patch = np.array((0, 0, w, h), np.int64)
            else:
                b, l = b[mask], l[mask]
                pf = patch.astype(np.float32)
                b = np.concatenate([np.maximum(b[:, :2], pf[:2]), np.minimum(b[:, 2:], pf[2:])], 1)
                b = b - np.tile(pf[:2], 2)
            geom[i] = k, left, top, patch[0], patch[1], patch[2], patch[3]
            cw, ch = int(patch[2] - patch[0]), int(patch[3] - patch[1])
            b = b * np.array([ow / cw, oh / ch, ow / cw, oh / ch], np.float32)           # Resize, then its clip
            b = np.stack([np.clip(b[:, 0], 0, ow), np.clip(b[:, 1], 0, oh), np.clip(b[:, 2], 0, ow), np.clip(b[:, 3], 0, oh)],
                         1).astype(np.float32)
            if prm['flip'][i]:
                b = np.stack([np.float32(ow) - b[:, 2], b[:, 1], np.float32(ow) - b[:, 0], b[:, 3]], 1)
            out_b.append(b.astype(np.float32))
            out_l.append(l)
        prm['geom'], prm['canvas'], prm['mode'] = geom, canvas, modes
        return out_b, out_l

    def records(self, desc, prm):
        """desc int64 [B, 3] (offset, h, w) + the draws, after boxes() chose the geometry -> [B] t3d_det_sample."""
        if 'geom' not in prm:
            raise RuntimeError('records() needs the geometry boxes() leaves in prm: call boxes() first')
        g = prm['geom']
        rec = np.zeros(len(desc), DET_SAMPLE_DTYPE)
        rec['offset'], rec['h'], rec['w'] = desc[:, 0], desc[:, 1], desc[:, 2]
        for j, f in enumerate(('turns', 'left', 'top', 'cx0', 'cy0', 'cx1', 'cy1')):
            rec[f] = g[:, j]
        rec['flags'] = (np.where(prm['flip'], DET_FLIP, 0) | np.where(prm['bright'], DET_BRIGHTNESS, 0)
                        | np.where(prm['contrast'], DET_CONTRAST, 0) | np.where(prm['contrast'] & ~prm['first'], DET_CONTRAST_LAST, 0)
                        | (DET_HSV if self.photo is not None else 0) | np.where(prm['sat_on'], DET_SATURATION, 0)
                        | np.where(prm['hue_on'], DET_HUE, 0))
        rec['delta'] = np.where(prm['bright'], prm['delta'], 0)
        rec['alpha'] = np.where(prm['contrast'], prm['alpha'], 1)
        rec['sat'] = np.where(prm['sat_on'], prm['sat'], 1)
        rec['hue'] = np.where(prm['hue_on'], prm['hue'], 0)
        rec['perm'] = prm['perm']
        return rec
