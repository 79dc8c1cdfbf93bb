"""The reference's Objectron dataset and its augmentation pipeline, with the pixel work on the GPU.

`Objectron` (dataloaders/objectron_main.py:14-137) reads the COCO-style annotations, filters the categories and cuts each
object out of its frame around the nine annotated keypoints.  Its `__getitem__` stays on the host -- it runs in DataLoader
workers -- and stops at the crop: it returns the sliced crop (uint8 RGB, decoded with Pillow), the keypoints shifted into
it and the class.  Resize, flip, brightness / contrast, rotation and the channel order are what `build_augmentations`
compiles the config's pipeline into: a per-sample record for one `t3d_augment_crops_u8` launch per batch
(csrc/augment.hip, driven by dataloaders/gpu_loader.py) plus the matching keypoint arithmetic, done here in float64.

Random draws happen in the main process, one numpy Generator per (seed, epoch, rank, batch): batches are reproducible and
do not depend on the number of workers.  The reference draws inside its workers with `random`, so its random stream is
not reproduced.

Keypoint conventions follow the albumentations of the reference's era (0.5 - 1.3; its test() still uses
IAAPiecewiseAffine): Resize scales by (ow / w, oh / h), HorizontalFlip maps x -> (ow - 1) - x, RandomRotate applies
the same 2x3 matrix as the image (cv.transform), ToTensor divides by (w, h) of its img_shape.  Albumentations and OpenCV
are not dependencies, so these conventions are UNPINNED against the libraries themselves; so is the JPEG decoder
(Pillow here, cv.imread in the reference).
"""
import json
import math
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from ..utils import OBJECTRON_CLASSES
from .gpu_crops import crop_cords_from_keypoints

__all__ = ['Objectron', 'AugmentPipeline', 'build_augmentations', 'collate_crops', 'AUG_SAMPLE_DTYPE']

# include/t3d.h: t3d_aug_sample (80 bytes) and its flags
AUG_SAMPLE_DTYPE = np.dtype([('offset', '<i8'), ('h', '<i4'), ('w', '<i4'), ('flags', '<i4'), ('alpha', '<f4'),
                             ('beta255', '<f4'), ('reserved', '<i4'), ('m', '<f8', (6,))])
assert AUG_SAMPLE_DTYPE.itemsize == 80
AUG_FLIP, AUG_LUT, AUG_ROTATE, AUG_SWAP_RB = 1, 2, 4, 8


class Objectron(torch.utils.data.Dataset):
    def __init__(self, root_folder, mode='train', transform=None, debug_mode=False, name='0', category_list='all'):
        self.root_folder = root_folder
        self.name = name
        self.transform = transform          # an AugmentPipeline: applied on the GPU by the loader, not here
        self.debug_mode = debug_mode        # (the reference's debug drawing needs cv2: not done)
        self.mode = mode
        self.num_classes = len(category_list) if isinstance(category_list, list) else len(OBJECTRON_CLASSES)
        if mode == 'train':
            ann_path = Path(root_folder).resolve() / 'annotations/objectron_train.json'
        elif mode in ('val', 'test'):
            ann_path = Path(root_folder).resolve() / 'annotations/objectron_test.json'
        else:
            raise RuntimeError('Unknown dataset mode')
        with open(ann_path, 'r') as f:
            self.ann = json.load(f)
        if category_list != 'all':
            self.annotations = [a for a in self.ann['annotations']
                                if OBJECTRON_CLASSES[a['category_id'] - 1] in category_list]
            images_id = {a['image_id'] for a in self.annotations}
            self.images = {img['id']: img for img in self.ann['images'] if img['id'] in images_id}
            assert len(self.images) == len(images_id)
        else:
            self.annotations = self.ann['annotations']
            self.images = self.ann['images']          # indexed by image id, as the reference does

    def __len__(self):
        return len(self.annotations)

    def category(self, indx):
        cat_id = int(self.annotations[indx]['category_id']) - 1
        # in case when classes are not equal to 9 choose closest
        return min(range(self.num_classes), key=lambda x: abs(x - cat_id))

    def load_image(self, indx):
        img_id = self.annotations[indx]['image_id']
        img_path = self.root_folder + '/' + self.images[img_id]['file_name']
        with Image.open(img_path) as im:
            return np.asarray(im.convert('RGB'))

    def __getitem__(self, indx):
        """-> (crop uint8 [h, w, 3] RGB, keypoints float64 [9, 2] in crop pixels, class); in test mode
        (frame, crop, keypoints, class, crop_cords) like objectron_main.py:93-96."""
        image = self.load_image(indx)
        kp = np.asarray(self.annotations[indx]['keypoints'], dtype=np.float64).reshape(9, 2)
        cropped_keypoints, cropped_img, crop_cords = self.crop(image, kp)
        category = self.category(indx)
        if self.mode == 'test':
            return image, cropped_img, cropped_keypoints, category, crop_cords
        return cropped_img, cropped_keypoints, category

    @staticmethod
    def crop(image, keypoints):
        """objectron_main.py:98-126: A.Crop is a numpy slice at the integer box."""
        real_h, real_w, _ = image.shape
        clipped, (x0, y0, x1, y1) = crop_cords_from_keypoints(keypoints, real_w, real_h)
        x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
        return clipped - np.asarray([x0, y0], clipped.dtype), image[y0:y1, x0:x1], (x0, y0, x1, y1)


def collate_crops(items):
    """DataLoader collate: variable-size crops packed into one uint8 buffer with a descriptor table.
    -> (packed uint8 [bytes], desc int64 [B, 3] = (offset, h, w), keypoints float64 [B, 9, 2], classes int64 [B]).
    Test-mode items drop their frame and crop box here (Evaluator.visual_test reads them from `.dataset`)."""
    if len(items[0]) == 5:
        items = [(c, k, cat) for _, c, k, cat, _ in items]
    desc = np.zeros((len(items), 3), np.int64)
    off = 0
    for i, (c, _, _) in enumerate(items):
        desc[i] = off, c.shape[0], c.shape[1]
        off += c.shape[0] * c.shape[1] * 3
    packed = np.empty(max(off, 1), np.uint8)
    for (c, _, _), (o, h, w) in zip(items, desc):
        packed[o:o + h * w * 3].reshape(h, w, 3)[...] = c
    kp = np.stack([np.asarray(k, np.float64) for _, k, _ in items])
    cats = np.asarray([int(cat) for _, _, cat in items], np.int64)
    return torch.from_numpy(packed), torch.from_numpy(desc), torch.from_numpy(kp), torch.from_numpy(cats)


def _to_tuple(v, bias=None):
    """albumentations.core.transforms_interface.to_tuple."""
    if isinstance(v, (int, float)):
        lo, hi = -v, v
    else:
        lo, hi = v
    if bias is not None:
        lo, hi = lo + bias, hi + bias
    return float(lo), float(hi)


def scale_by_angle(angle, h, w):
    """RandomRotate._get_scale_by_angle (utils/transforms.py:71-78)."""
    rad_angle = math.radians(angle)
    cos = math.cos(rad_angle) - 1
    sin = math.sin(rad_angle)
    delta_h = w / 2 * cos + h / 2 * sin
    delta_w = w / 2 * sin + h / 2 * cos
    return max(w / (w + 2 * abs(delta_w)), h / (h + 2 * abs(delta_h)))


def rotation_matrix(angle, h, w):
    """cv.getRotationMatrix2D((w / 2, h / 2), angle, scale) in fp64, OpenCV's operation order."""
    scale = scale_by_angle(angle, h, w)
    a = angle * (math.pi / 180)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = w * 0.5, h * 0.5
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def invert_affine(M):
    """The inversion cv::warpAffine applies to a forward matrix (imgwarp.cpp), same operation order."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(-1)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1. / D if D != 0 else 0.
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, np.float64).reshape(2, 3)


_KNOWN = ('convert_color', 'resize', 'horizontal_flip', 'random_brightness_contrast', 'random_rotate', 'normalize',
          'to_tensor')


class AugmentPipeline:
    """A compiled `cfg.*_data_pipeline`: the output size, the per-sample random draws, the kernel records and the keypoint
    arithmetic.  The kernel's order is resize -> flip -> brightness/contrast -> rotate (flip and the LUT commute)."""

    def __init__(self, steps, normalization):
        names = [str(t) for t, _ in steps]
        for t in names:
            if t not in _KNOWN:
                raise NotImplementedError(f'transform {t!r} is not built for the GPU pipeline (built: {", ".join(_KNOWN)})')
        for t in set(names):
            if names.count(t) > 1:
                raise NotImplementedError(f'transform {t!r} appears {names.count(t)} times; the GPU pipeline applies it once')
        args = {t: dict(a or {}) for t, a in steps}
        pos = {t: i for i, t in enumerate(names)}
        if 'resize' not in pos:
            raise ValueError('the pipeline needs a resize: crops of different sizes cannot be batched')
        for t in ('horizontal_flip', 'random_brightness_contrast', 'random_rotate', 'normalize', 'to_tensor'):
            if t in pos and pos[t] < pos['resize']:
                raise NotImplementedError(f'{t} before resize is not built (the kernel resizes first)')
        if 'random_rotate' in pos:
            for t in ('horizontal_flip', 'random_brightness_contrast'):
                if t in pos and pos[t] > pos['random_rotate']:
                    raise NotImplementedError(f'{t} after random_rotate is not built (the kernel rotates last)')
        if 'normalize' not in pos:
            raise ValueError('the pipeline needs normalize: the model normalises its uint8 input with cfg.data.normalization')
        if 'to_tensor' not in pos:
            raise ValueError('the pipeline needs to_tensor (the keypoints are normalised by its img_shape)')
        for t in ('convert_color', 'horizontal_flip', 'random_brightness_contrast', 'random_rotate'):
            if t in pos and pos[t] > pos['normalize']:
                raise NotImplementedError(f'{t} after normalize is not built (the kernel works on uint8 images)')
        self.swap = 'convert_color' not in pos          # cv.imread gives BGR; without convert_color the model sees BGR

        r = args['resize']
        if int(r.get('interpolation', 1)) != 1:
            raise NotImplementedError('resize: only interpolation=cv.INTER_LINEAR (1) is built')
        self.size = (int(r['height']), int(r['width']))                     # (oh, ow): A.Resize(height, width)
        self.p_flip = self._p(args.get('horizontal_flip'), 0.5)
        rbc = args.get('random_brightness_contrast')
        self.p_lut = self._p(rbc, 0.5)
        if rbc is not None and not rbc.get('brightness_by_max', True):
            raise NotImplementedError('random_brightness_contrast: only brightness_by_max=True is built')
        self.blim = _to_tuple(rbc.get('brightness_limit', 0.2) if rbc else 0.2)
        self.clim = _to_tuple(rbc.get('contrast_limit', 0.2) if rbc else 0.2)
        rot = args.get('random_rotate')
        self.p_rot = self._p(rot, 0.5)
        if rot is not None and int(rot.get('interpolation', 1)) != 1:
            raise NotImplementedError('random_rotate: only interpolation=cv.INTER_LINEAR (1) is built')
        self.alim = _to_tuple(rot.get('angle_limit', 0.1) if rot else 0.1)
        nm = args['normalize']
        mean, std = list(nm.get('mean', (0.485, 0.456, 0.406))), list(nm.get('std', (0.229, 0.224, 0.225)))
        if float(nm.get('max_pixel_value', 255.0)) != 255.0:
            raise ValueError('normalize: only max_pixel_value=255 is built')
        if normalization is None or [float(v) for v in mean] != [float(v) for v in normalization['mean']] \
                or [float(v) for v in std] != [float(v) for v in normalization['std']]:
            raise ValueError(f'normalize (mean={mean}, std={std}) must equal cfg.data.normalization ({normalization}): the '
                             'model normalises its uint8 input inside the stem with those values')
        self.img_shape = tuple(int(v) for v in args['to_tensor']['img_shape'])[:2]          # (h, w)

    @staticmethod
    def _p(a, default):
        if a is None:
            return 0.0
        return 1.0 if a.get('always_apply', False) else float(a.get('p', default))

    @property
    def is_random(self):
        return self.p_flip > 0 or self.p_lut > 0 or self.p_rot > 0

    def draw(self, n, key):
        """Per-sample parameters for n samples from numpy Generator(key) (key = (seed, epoch, rank, batch[, item])).
        -> dict of arrays: flip, lut, rot (bool), alpha, beta, angle (float64)."""
        u = np.random.default_rng([int(k) for k in key]).random((n, 6))
        (blo, bhi), (clo, chi), (alo, ahi) = self.blim, self.clim, self.alim
        return dict(flip=u[:, 0] < self.p_flip, lut=u[:, 1] < self.p_lut, alpha=1.0 + (clo + (chi - clo) * u[:, 2]),
                    beta=0.0 + (blo + (bhi - blo) * u[:, 3]), rot=u[:, 4] < self.p_rot, angle=alo + (ahi - alo) * u[:, 5])

    def records(self, desc, prm):
        """desc int64 [B, 3] (offset, h, w) + draws -> t3d_aug_sample records (numpy structured [B])."""
        oh, ow = self.size
        B = len(desc)
        rec = np.zeros(B, AUG_SAMPLE_DTYPE)
        rec['offset'], rec['h'], rec['w'] = desc[:, 0], desc[:, 1], desc[:, 2]
        flags = np.where(prm['flip'], AUG_FLIP, 0) | np.where(prm['lut'], AUG_LUT, 0) | np.where(prm['rot'], AUG_ROTATE, 0)
        rec['flags'] = flags | (AUG_SWAP_RB if self.swap else 0)
        rec['alpha'] = np.where(prm['lut'], prm['alpha'], 1.0).astype(np.float32)
        rec['beta255'] = np.where(prm['lut'], (prm['beta'] * 255).astype(np.float32), 0.0)
        for i in np.nonzero(prm['rot'])[0]:
            rec['m'][i] = invert_affine(rotation_matrix(float(prm['angle'][i]), oh, ow)).reshape(-1)
        return rec

    def keypoints(self, kp, desc, prm):
        """Keypoints in crop pixels (float64 [B, 9, 2]) -> the loader's float32 [B, 9, 2], normalised like ToTensor."""
        oh, ow = self.size
        kp = np.array(kp, np.float64)
        h, w = desc[:, 1].astype(np.float64), desc[:, 2].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            x, y = kp[..., 0] * (ow / w)[:, None], kp[..., 1] * (oh / h)[:, None]
        x = np.where(prm['flip'][:, None], (ow - 1) - x, x)
        for i in np.nonzero(prm['rot'])[0]:
            m = rotation_matrix(float(prm['angle'][i]), oh, ow).reshape(-1)
            x[i], y[i] = m[0] * x[i] + m[1] * y[i] + m[2], m[3] * x[i] + m[4] * y[i] + m[5]
        th, tw = self.img_shape
        return (np.stack([x, y], -1) / np.asarray([tw, th], np.float32)).astype(np.float32)


def build_augmentations(cfg):
    """builders/loader_builder.py:62-68 -> (train, test) compiled pipelines."""
    norm = cfg.data.normalization or None
    return (AugmentPipeline(cfg.train_data_pipeline, norm), AugmentPipeline(cfg.test_data_pipeline, norm))
