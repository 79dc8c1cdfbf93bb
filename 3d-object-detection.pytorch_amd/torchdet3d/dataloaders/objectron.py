"""The reference's Objectron dataset and its augmentation pipeline, with the pixel work on the GPU.

`Objectron` (dataloaders/objectron_main.py:14-137) reads the COCO-style annotations, filters the categories and cuts each
object out of its frame around the nine annotated keypoints.  Its `__getitem__` stays on the host -- it runs in DataLoader
workers -- and stops at the crop: it returns the sliced crop (uint8 RGB, decoded with Pillow), the keypoints shifted into
it and the class.  Resize, flip, brightness / contrast, rotation and the channel order are what `build_augmentations`
compiles the config's pipeline into: a per-sample record for one `t3d_augment_crops_u8` launch per batch
(csrc/augment.hip, driven by dataloaders/gpu_loader.py) plus the matching keypoint arithmetic, done here in float64.
A pipeline that also names random_rescale, hue_saturation_value or color_jitter compiles into the same records plus one
`t3d_aug_chain` record per sample -- the colour ops in the config's order and the second warp -- for
`t3d_augment_chain_crops_u8` (csrc/augment_chain.hip); the default pipeline's draws, records and launches do not change.

Random draws happen in the main process, one numpy Generator per (seed, epoch, rank, batch): batches are reproducible and
do not depend on the number of workers.  The reference draws inside its workers with `random`, so its random stream is
not reproduced.

Keypoint conventions follow the albumentations of the reference's era (0.5 - 1.3; its test() still uses
IAAPiecewiseAffine): Resize scales by (ow / w, oh / h), HorizontalFlip maps x -> (ow - 1) - x, RandomRotate applies
the same 2x3 matrix as the image (cv.transform), ToTensor divides by (w, h) of its img_shape.  Albumentations and OpenCV
are not dependencies, so these conventions are UNPINNED against the libraries themselves; so is the JPEG decoder
(Pillow here, cv.imread in the reference).
"""
import itertools
import json
import math
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from ..utils import OBJECTRON_CLASSES
from .gpu_crops import crop_cords_from_keypoints

__all__ = ['Objectron', 'AugmentPipeline', 'build_augmentations', 'collate_crops', 'AUG_SAMPLE_DTYPE', 'AUG_CHAIN_DTYPE',
           'chain_stages', 'chain_scratch_bytes', 'resize_records']

# include/t3d.h: t3d_aug_sample (80 bytes) and its flags
AUG_SAMPLE_DTYPE = np.dtype([('offset', '<i8'), ('h', '<i4'), ('w', '<i4'), ('flags', '<i4'), ('alpha', '<f4'),
                             ('beta255', '<f4'), ('reserved', '<i4'), ('m', '<f8', (6,))])
assert AUG_SAMPLE_DTYPE.itemsize == 80
AUG_FLIP, AUG_LUT, AUG_ROTATE, AUG_SWAP_RB = 1, 2, 4, 8
# include/t3d.h: t3d_aug_chain (280 bytes), its op kinds, its flag and the stages of t3d_augment_chain_*_u8
CHAIN_MAX_OPS = 8
AUG_CHAIN_DTYPE = np.dtype([('n_ops', '<i4'), ('flags', '<i4'), ('kind', '<i4', (CHAIN_MAX_OPS,)), ('p', '<f8', (CHAIN_MAX_OPS, 3)),
                            ('m2', '<f8', (6,))])
assert AUG_CHAIN_DTYPE.itemsize == 280
CHAIN_LUT, CHAIN_HSV, CHAIN_BRIGHTNESS, CHAIN_CONTRAST, CHAIN_SATURATION, CHAIN_HUE = 1, 2, 3, 4, 5, 6
CHAIN_WARP2 = 1
STAGE_MEAN, STAGE_WARP, STAGE_WARP2 = 1, 2, 4
# The second generator of a pipeline with a new transform is keyed (*key, _CHAIN_TAG): one component longer than a batch
# key, and no item index -- the last component of an item key -- reaches the tag, so it equals no key the loader draws with.
_CHAIN_TAG = 0x7C4A1F3B9D5E
_JITTER_ORDERS = np.array(list(itertools.permutations(range(4))), np.int64)      # 24 orders of (b, c, s, h)


def resize_records(desc):
    """desc [B, 3] = (offset, h, w) of the source images -> their t3d_aug_sample records with no flag set: the resize alone."""
    rec = np.zeros(len(desc), AUG_SAMPLE_DTYPE)
    rec['offset'], rec['h'], rec['w'] = desc[:, 0], desc[:, 1], desc[:, 2]
    return rec


def chain_stages(rec, ext):
    """The `stages` argument of t3d_augment_chain_*_u8 for a batch of records: which passes some sample needs."""
    n = np.arange(CHAIN_MAX_OPS)[None] < ext['n_ops'][:, None]
    return ((STAGE_MEAN if (n & (ext['kind'] == CHAIN_CONTRAST)).any() else 0)
            | (STAGE_WARP if (rec['flags'] & AUG_ROTATE).any() else 0)
            | (STAGE_WARP2 if (ext['flags'] & CHAIN_WARP2).any() else 0))


def chain_scratch_bytes(B, oh, ow, stages):
    """include/t3d.h: the grey sums plus one uint8 image batch per warp stage."""
    return 8 * B + (bool(stages & STAGE_WARP) + bool(stages & STAGE_WARP2)) * ((B * oh * ow * 3 + 7) // 8 * 8)


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


def rotation_matrix(angle, h, w, scale=None):
    """cv.getRotationMatrix2D((w / 2, h / 2), angle, scale) in fp64, OpenCV's operation order.  scale None: RandomRotate's
    `scale_by_angle`; RandomRescale passes angle 0 and its own scale (utils/transforms.py:31-35)."""
    if scale is None:
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
          'to_tensor', 'random_rescale', 'hue_saturation_value', 'color_jitter')
_COLOUR = ('random_brightness_contrast', 'hue_saturation_value', 'color_jitter')
_WARPS = ('random_rescale', 'random_rotate')
_CHAINED = ('random_rescale', 'hue_saturation_value', 'color_jitter')      # what csrc/augment_chain.hip is needed for


def _jitter_range(name, v, offset, bounds, clip):
    """albumentations' ColorJitter.__check_values: a scalar v -> [offset - v, offset + v] (the lower end clipped at 0 for
    brightness / contrast / saturation), a pair as it is; anything outside `bounds` is refused."""
    if isinstance(v, (int, float)):
        if v < 0:
            raise ValueError(f'color_jitter: {name} = {v} must be non-negative')
        lo, hi = offset - v, offset + v
        if clip:
            lo = max(lo, 0)
    elif isinstance(v, (tuple, list)) and len(v) == 2:
        lo, hi = v
    else:
        raise ValueError(f'color_jitter: {name} = {v!r} must be a number or a pair')
    if not bounds[0] <= lo <= hi <= bounds[1]:
        raise ValueError(f'color_jitter: {name} = {v!r} gives [{lo}, {hi}], outside {list(bounds)}')
    return float(lo), float(hi)


class AugmentPipeline:
    """A compiled `cfg.*_data_pipeline`: the output size, the per-sample random draws, the kernel records and the keypoint
    arithmetic.  The kernel's order is resize -> flip -> brightness/contrast -> rotate (flip and the LUT commute).
    Accepted: [convert_color] resize {horizontal_flip | colour ops}* {random_rescale | random_rotate}* normalize to_tensor;
    the colour ops (random_brightness_contrast, hue_saturation_value, color_jitter) and the two warps are applied in the
    config's order, and the flip commutes with every colour op.  `chained`: the pipeline names one of random_rescale,
    hue_saturation_value, color_jitter and runs through t3d_augment_chain_*_u8."""

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
        for t in ('horizontal_flip',) + _COLOUR + _WARPS + ('normalize', 'to_tensor'):
            if t in pos and pos[t] < pos['resize']:
                raise NotImplementedError(f'{t} before resize is not built (the kernel resizes first)')
        for warp in _WARPS:
            for t in ('horizontal_flip',) + _COLOUR:
                if warp in pos and t in pos and pos[t] > pos[warp]:
                    raise NotImplementedError(f'{t} after {warp} is not built (the kernel warps last)')
        if 'normalize' not in pos:
            raise ValueError('the pipeline needs normalize: the model normalises its uint8 input with cfg.data.normalization')
        if 'to_tensor' not in pos:
            raise ValueError('the pipeline needs to_tensor (the keypoints are normalised by its img_shape)')
        for t in ('convert_color', 'horizontal_flip') + _COLOUR + _WARPS:
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
        # the three transforms of csrc/augment_chain.hip; arguments as the reference's classes parse them
        self.chained = any(t in pos for t in _CHAINED)
        self.colour_order = [t for t in names if t in _COLOUR]
        self.warp_order = [t for t in names if t in _WARPS]
        rs = args.get('random_rescale')
        self.p_rescale = self._p(rs, 0.5)
        if rs is not None and int(rs.get('interpolation', 1)) != 1:
            raise NotImplementedError('random_rescale: only interpolation=cv.INTER_LINEAR (1) is built')
        # RandomRescale: to_tuple(scale_limit, bias=0) -- with the default 0.1 the scale is drawn from (-0.1, 0.1), the
        # reference's quirk, restated as it is
        self.slim = _to_tuple(rs.get('scale_limit', 0.1) if rs else 0.1, bias=0)
        hsv = args.get('hue_saturation_value')
        self.p_hsv = self._p(hsv, 0.5)
        self.hsv_lim = tuple(_to_tuple(hsv.get(k, d) if hsv else d)
                             for k, d in (('hue_shift_limit', 20), ('sat_shift_limit', 30), ('val_shift_limit', 20)))
        cj = args.get('color_jitter')
        self.p_jit = self._p(cj, 0.5)
        self.jit_lim = tuple(_jitter_range(k, cj.get(k, 0.2) if cj else 0.2, off, bounds, clip) for k, off, bounds, clip in
                             (('brightness', 1, (0, float('inf')), True), ('contrast', 1, (0, float('inf')), True),
                              ('saturation', 1, (0, float('inf')), True), ('hue', 0, (-0.5, 0.5), False)))
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
        return self.p_flip > 0 or self.p_lut > 0 or self.p_rot > 0 or self.p_rescale > 0 or self.p_hsv > 0 or self.p_jit > 0

    def draw(self, n, key):
        """Per-sample parameters for n samples from numpy Generator(key) (key = (seed, epoch, rank, batch[, item])).
        -> dict of arrays: flip, lut, rot (bool), alpha, beta, angle (float64).
        A chained pipeline adds, from a second Generator keyed (*key, _CHAIN_TAG) -- the six columns above are what they
        are without it -- `random((n, 12))` with the columns
          0 rescale fired    1 scale                       2 hue_saturation_value fired    3, 4, 5 hue / sat / val shift
          6 color_jitter fired    7, 8, 9, 10 brightness / contrast / saturation / hue factor
          11 the jitter order: floor(24 u) indexes itertools.permutations(range(4)) of (brightness, contrast, saturation, hue)
        -> rescale, hsv, jit (bool), scale, dh, ds, dv, jb, jc, js, jh (float64), order (int64 [n, 4]: the ops in
        application order)."""
        u = np.random.default_rng([int(k) for k in key]).random((n, 6))
        (blo, bhi), (clo, chi), (alo, ahi) = self.blim, self.clim, self.alim
        prm = dict(flip=u[:, 0] < self.p_flip, lut=u[:, 1] < self.p_lut, alpha=1.0 + (clo + (chi - clo) * u[:, 2]),
                   beta=0.0 + (blo + (bhi - blo) * u[:, 3]), rot=u[:, 4] < self.p_rot, angle=alo + (ahi - alo) * u[:, 5])
        if self.chained:
            v = np.random.default_rng([int(k) for k in key] + [_CHAIN_TAG]).random((n, 12))

            def lin(lim, col):
                return lim[0] + (lim[1] - lim[0]) * v[:, col]
            prm.update(rescale=v[:, 0] < self.p_rescale, scale=lin(self.slim, 1), hsv=v[:, 2] < self.p_hsv,
                       dh=lin(self.hsv_lim[0], 3), ds=lin(self.hsv_lim[1], 4), dv=lin(self.hsv_lim[2], 5),
                       jit=v[:, 6] < self.p_jit, jb=lin(self.jit_lim[0], 7), jc=lin(self.jit_lim[1], 8),
                       js=lin(self.jit_lim[2], 9), jh=lin(self.jit_lim[3], 10),
                       order=_JITTER_ORDERS[np.minimum((v[:, 11] * 24).astype(np.int64), 23)])
        return prm

    def _warps(self, prm, i):
        """The forward matrices of the warps that fire on sample i, in the config's order."""
        oh, ow = self.size
        out = []
        for t in self.warp_order:
            if t == 'random_rotate' and prm['rot'][i]:
                out.append(rotation_matrix(float(prm['angle'][i]), oh, ow))
            elif t == 'random_rescale' and prm['rescale'][i]:
                out.append(rotation_matrix(0.0, oh, ow, float(prm['scale'][i])))
        return out

    def records(self, desc, prm):
        """desc int64 [B, 3] (offset, h, w) + draws -> t3d_aug_sample records (numpy structured [B]); a chained pipeline
        -> (t3d_aug_sample records, t3d_aug_chain records)."""
        if self.chained:
            return self._chain_records(desc, prm)
        oh, ow = self.size
        B = len(desc)
        rec = resize_records(desc)
        flags = np.where(prm['flip'], AUG_FLIP, 0) | np.where(prm['lut'], AUG_LUT, 0) | np.where(prm['rot'], AUG_ROTATE, 0)
        rec['flags'] = flags | (AUG_SWAP_RB if self.swap else 0)
        rec['alpha'] = np.where(prm['lut'], prm['alpha'], 1.0).astype(np.float32)
        rec['beta255'] = np.where(prm['lut'], (prm['beta'] * 255).astype(np.float32), 0.0)
        for i in np.nonzero(prm['rot'])[0]:
            rec['m'][i] = invert_affine(rotation_matrix(float(prm['angle'][i]), oh, ow)).reshape(-1)
        return rec

    def _chain_records(self, desc, prm):
        """The base record carries the flip, the channel order and the FIRST warp that fires; the brightness / contrast LUT
        goes into the colour program, at its place in the config's order."""
        B = len(desc)
        rec, ext = resize_records(desc), np.zeros(B, AUG_CHAIN_DTYPE)
        rec['flags'] = np.where(prm['flip'], AUG_FLIP, 0) | (AUG_SWAP_RB if self.swap else 0)
        rec['alpha'] = 1.0
        jitter = (('jb', CHAIN_BRIGHTNESS), ('jc', CHAIN_CONTRAST), ('js', CHAIN_SATURATION), ('jh', CHAIN_HUE))
        for i in range(B):
            ops = []
            for t in self.colour_order:
                if t == 'random_brightness_contrast' and prm['lut'][i]:
                    ops.append((CHAIN_LUT, float(np.float32(prm['alpha'][i])), float((prm['beta'][i] * 255).astype(np.float32))))
                elif t == 'hue_saturation_value' and prm['hsv'][i]:
                    ops.append((CHAIN_HSV, prm['dh'][i], prm['ds'][i], prm['dv'][i]))
                elif t == 'color_jitter' and prm['jit'][i]:
                    ops += [(jitter[k][1], prm[jitter[k][0]][i]) for k in prm['order'][i]]
            ext['n_ops'][i] = len(ops)
            for k, (kind, *p) in enumerate(ops):
                ext['kind'][i, k] = kind
                ext['p'][i, k, :len(p)] = p
            warps = self._warps(prm, i)
            if warps:
                rec['flags'][i] |= AUG_ROTATE
                rec['m'][i] = invert_affine(warps[0]).reshape(-1)
            if len(warps) > 1:
                ext['flags'][i] = CHAIN_WARP2
                ext['m2'][i] = invert_affine(warps[1]).reshape(-1)
        return rec, ext

    def keypoints(self, kp, desc, prm):
        """Keypoints in crop pixels (float64 [B, 9, 2]) -> the loader's float32 [B, 9, 2], normalised like ToTensor."""
        oh, ow = self.size
        kp = np.array(kp, np.float64)
        h, w = desc[:, 1].astype(np.float64), desc[:, 2].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            x, y = kp[..., 0] * (ow / w)[:, None], kp[..., 1] * (oh / h)[:, None]
        x = np.where(prm['flip'][:, None], (ow - 1) - x, x)
        if self.chained:
            for i in range(len(kp)):
                for m in self._warps(prm, i):
                    m = m.reshape(-1)
                    x[i], y[i] = m[0] * x[i] + m[1] * y[i] + m[2], m[3] * x[i] + m[4] * y[i] + m[5]
        else:
            for i in np.nonzero(prm['rot'])[0]:
                m = rotation_matrix(float(prm['angle'][i]), oh, ow).reshape(-1)
                x[i], y[i] = m[0] * x[i] + m[1] * y[i] + m[2], m[3] * x[i] + m[4] * y[i] + m[5]
        th, tw = self.img_shape
        return (np.stack([x, y], -1) / np.asarray([tw, th], np.float32)).astype(np.float32)


def build_augmentations(cfg):
    """builders/loader_builder.py:62-68 -> (train, test) compiled pipelines."""
    norm = cfg.data.normalization or None
    return (AugmentPipeline(cfg.train_data_pipeline, norm), AugmentPipeline(cfg.test_data_pipeline, norm))
