"""Test helper (not a test module): numpy restatements of the reference's crop pipeline steps that csrc/augment.hip runs,
and a tiny Objectron-style dataset writer.

  * `lut_u8`            albumentations' brightness_contrast_adjust on uint8 (brightness_by_max=True): float32 LUT, clipped,
                        truncated.
  * `rotation_matrix`   cv.getRotationMatrix2D((w/2, h/2), angle, RandomRotate._get_scale_by_angle(angle, h, w)).
  * `warp_affine_u8`    cv.warpAffine(img, M, (w, h), INTER_LINEAR), border constant 0, OpenCV's 8-bit fixed-point path:
                        inverse map, AB_BITS = 10, INTER_BITS = 5, 15-bit remap weights.  `warp_affine_float` is the
                        textbook fp64 bilinear it is checked against.
  * `augment`           resize -> flip -> LUT -> rotate -> channel swap, rounded to uint8 where the reference stores uint8.
  * `keypoints`         the float64 keypoint arithmetic of the same steps, then ToTensor's division, cast to float32.
OpenCV / albumentations are not available: parity with the libraries themselves is unpinned."""
import json
import math
import os

import numpy as np

from oracle.crop_resize import resize_linear_u8


def lut_u8(alpha, beta):
    lut = np.arange(0, 256).astype('float32')
    if alpha != 1:
        lut *= alpha
    if beta != 0:
        lut += beta * 255
    return np.clip(lut, 0, 255).astype(np.uint8)


def rotation_matrix(angle, h, w):
    rad = math.radians(angle)
    cos, sin = math.cos(rad) - 1, math.sin(rad)
    delta_h = w / 2 * cos + h / 2 * sin
    delta_w = w / 2 * sin + h / 2 * cos
    scale = max(w / (w + 2 * abs(delta_w)), h / (h + 2 * abs(delta_h)))
    a = angle * (math.pi / 180)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = w * 0.5, h * 0.5
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])


def invert_affine(M):
    (m0, m1, m2), (m3, m4, m5) = [[float(v) for v in r] for r in M]
    D = m0 * m4 - m1 * m3
    D = 1. / D if D != 0 else 0.
    a11, a12, a21, a22 = m4 * D, m1 * -D, m3 * -D, m0 * D
    return np.array([[a11, a12, -a11 * m2 - a12 * m5], [a21, a22, -a21 * m2 - a22 * m5]])


def _taps(img, sx, sy):
    h, w = img.shape[:2]
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    v = img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(np.int64)
    return np.where(ok[..., None], v, 0)


def warp_affine_u8(img, M):
    """Forward matrix M (2x3) -> warped uint8 image of the same size."""
    h, w = img.shape[:2]
    m = invert_affine(M).reshape(-1)
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    adelta, bdelta = np.rint(m[0] * x * 1024).astype(np.int64), np.rint(m[3] * x * 1024).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024).astype(np.int64) + 16
    X, Y = (X0[:, None] + adelta[None]) >> 5, (Y0[:, None] + bdelta[None]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = (X & 31)[..., None], (Y & 31)[..., None]
    acc = (_taps(img, sx, sy) * ((32 - fy) * (32 - fx) * 32) + _taps(img, sx + 1, sy) * ((32 - fy) * fx * 32)
           + _taps(img, sx, sy + 1) * (fy * (32 - fx) * 32) + _taps(img, sx + 1, sy + 1) * (fy * fx * 32))
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def warp_affine_float(img, M):
    """Textbook bilinear warp in fp64 (exact inverse map, zero outside), unrounded."""
    h, w = img.shape[:2]
    m = np.linalg.inv(np.vstack([M, [0, 0, 1]]))[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy = m[0, 0] * xx + m[0, 1] * yy + m[0, 2], m[1, 0] * xx + m[1, 1] * yy + m[1, 2]
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
    return (_taps(img, x0, y0) * (1 - fx) * (1 - fy) + _taps(img, x0 + 1, y0) * fx * (1 - fy)
            + _taps(img, x0, y0 + 1) * (1 - fx) * fy + _taps(img, x0 + 1, y0 + 1) * fx * fy)


def augment(crop, oh, ow, flip=False, alpha=1.0, beta=0.0, angle=None, swap=False):
    img = resize_linear_u8(crop, (ow, oh))
    if flip:
        img = img[:, ::-1]
    if alpha != 1.0 or beta != 0.0:
        img = lut_u8(alpha, beta)[img]
    if angle is not None:
        img = warp_affine_u8(np.ascontiguousarray(img), rotation_matrix(angle, oh, ow))
    if swap:
        img = img[..., ::-1]
    return np.ascontiguousarray(img)


def keypoints(kp, h, w, oh, ow, flip=False, angle=None, img_shape=None):
    """kp [9, 2] in crop pixels -> float32 [9, 2] as A.Resize / HorizontalFlip / RandomRotate / ToTensor leave them."""
    out = []
    th, tw = img_shape or (oh, ow)
    M = rotation_matrix(angle, oh, ow) if angle is not None else None
    for x, y in np.asarray(kp, np.float64):
        x, y = x * (ow / w), y * (oh / h)
        if flip:
            x = (ow - 1) - x
        if M is not None:
            x, y = M[0, 0] * x + M[0, 1] * y + M[0, 2], M[1, 0] * x + M[1, 1] * y + M[1, 2]
        out.append((x, y))
    return (np.asarray(out) / np.asarray([tw, th], np.float32)).astype(np.float32)


def write_dataset(root, seed=0, n_train=12, n_test=6, cats=None):
    """A tiny Objectron-style dataset: 480x640 and 640x480 frames as PNG and JPEG, annotations/objectron_{train,test}.json
    (COCO layout; image ids are list positions, as the reference's category_list='all' path assumes)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    yy, xx = np.mgrid[0:640, 0:640]
    for split, n in (('train', n_train), ('test', n_test)):
        images, anns = [], []
        for i in range(n):
            H, W = ((480, 640), (640, 480))[i % 2]
            ext = ('png', 'jpg')[(i // 2) % 2]
            base = np.stack([127 + 100 * np.sin(xx[:H, :W] / (17.0 + i) + c) * np.cos(yy[:H, :W] / 23.0 - c) for c in range(3)], -1)
            frame = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
            name = f'images/{split}_{i}.{ext}'
            Image.fromarray(frame).save(os.path.join(root, name))
            images.append(dict(id=i, file_name=name, width=W, height=H))
            for k in range(1 + i % 2):
                c = rng.uniform([80, 80], [W - 80, H - 80])
                kp = c + rng.uniform(-70, 70, (9, 2)) * rng.uniform(0.5, 2.0)
                if k == 1:
                    kp[0] = (-20.0, H + 15.0)                       # a point outside the frame (clipped)
                cat = int(cats[len(anns) % len(cats)]) if cats else int(rng.integers(1, 10))
                anns.append(dict(id=len(anns), image_id=i, category_id=cat, keypoints=[float(v) for v in kp.reshape(-1)]))
        with open(os.path.join(root, 'annotations', f'objectron_{split}.json'), 'w') as f:
            json.dump(dict(images=images, annotations=anns, categories=[]), f)
    return root


NORMALIZATION = dict(mean=[0.5931, 0.4690, 0.4229], std=[0.2471, 0.2214, 0.2157])


def default_pipelines(size=(224, 224), norm=NORMALIZATION):
    """configs/default_config.py:31-42 of the reference, with `data.resize = size`."""
    train = [('convert_color', dict()),
             ('resize', dict(height=size[0], width=size[1])),
             ('horizontal_flip', dict(p=0.4)),
             ('random_brightness_contrast', dict(p=0.3)),
             ('random_rotate', dict(angle_limit=10., p=0.4)),
             ('normalize', norm),
             ('to_tensor', dict(img_shape=size))]
    test = [('convert_color', dict()),
            ('resize', dict(height=size[0], width=size[1])),
            ('normalize', norm),
            ('to_tensor', dict(img_shape=size))]
    return train, test
