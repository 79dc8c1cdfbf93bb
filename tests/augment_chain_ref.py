"""Test helper (not a test module): numpy restatement of the steps csrc/augment_chain.hip adds to the crop pipeline --
random_rescale, hue_saturation_value and color_jitter -- and of the whole chain around them.  The shared steps (resize,
LUT, fixed-point warp, rotation matrix) are tests/augment_ref.py's.

The formulas are recalled from the OpenCV 4.x and albumentations 1.x sources; neither library is available, so parity with
them is UNPINNED and this file is the project's definition.  Every step that yields an image yields uint8.

  * `rgb_to_hsv_u8`   cv.cvtColor(RGB2HSV) on 8-bit data, H in 0..179: integer arithmetic with the two 12-bit division tables.
  * `hsv_to_rgb_u8`   cv.cvtColor(HSV2RGB) on 8-bit data in float32, products and sums rounded separately, the byte is
                      rint(x * 255), half to even.  (s == 0 needs no case of its own: every table entry is v then.)
  * `hsv_shift`       albumentations' shift_hsv on uint8: H = mod(H + dh, 180), S / V = clip(. + d, 0, 255), in fp64, truncated.
  * `grey_u8`         cv.cvtColor(RGB2GRAY), 15-bit fixed point.
  * `brightness`, `contrast`, `saturation`, `hue`   albumentations' ColorJitter ops on uint8.  Deviation: `contrast` uses
                      the general LUT formula for every factor (albumentations returns the image itself at exactly 1 and the
                      rounded mean at exactly 0: measure zero in the draws).
  * `rescale_matrix`  cv.getRotationMatrix2D((w / 2, h / 2), 0, scale): RandomRescale (utils/transforms.py:20-47).
  * `chain`           resize -> flip -> colour ops in the given order -> warps in the given order -> channel swap.
  * `keypoints`       the fp64 keypoint arithmetic of the same steps, then ToTensor's division, cast to float32."""
import math

import numpy as np

import augment_ref as R

F32 = np.float32
_I = np.arange(256, dtype=np.float64)
with np.errstate(divide='ignore'):
    SDIV = np.where(_I > 0, np.rint((255 << 12) / _I), 0).astype(np.int64)
    HDIV = np.where(_I > 0, np.rint((180 << 12) / (6 * _I)), 0).astype(np.int64)
HSCALE, INV255 = F32(6) / F32(180), F32(1) / F32(255)
# OpenCV's sector table: (b, g, r) of sector k are tab[SECTOR[k]]
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def rgb_to_hsv_u8(img):
    """uint8 [..., 3] RGB -> uint8 [..., 3] (H 0..179, S, V)."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << 11)) >> 12                  # (arithmetic shift: h may be negative)
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], -1).astype(np.uint8)


def hsv_to_rgb_u8(hsv):
    """uint8 [..., 3] (H, S, V) -> uint8 [..., 3] RGB, float32 arithmetic."""
    hf = hsv[..., 0].astype(F32) * HSCALE
    s, v = hsv[..., 1].astype(F32) * INV255, hsv[..., 2].astype(F32) * INV255
    while (hf >= 6).any():                                  # (H beyond 179: OpenCV wraps the sector)
        hf = np.where(hf >= 6, hf - F32(6), hf).astype(F32)
    sector = np.floor(hf).astype(np.int64)
    f = (hf - sector.astype(F32)).astype(F32)
    one = F32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], -1)
    assert tab.dtype == F32
    bgr = np.take_along_axis(tab, SECTOR[sector], -1)
    out = np.clip(np.rint(bgr * F32(255)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


def hsv_shift(img, dh, ds, dv):
    hsv = rgb_to_hsv_u8(img).astype(np.float64)
    h = np.mod(hsv[..., 0] + float(dh), 180.0)
    s = np.clip(hsv[..., 1] + float(ds), 0, 255)
    v = np.clip(hsv[..., 2] + float(dv), 0, 255)
    return hsv_to_rgb_u8(np.stack([h, s, v], -1).astype(np.uint8))


def grey_u8(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((9798 * r + 19235 * g + 3735 * b + (1 << 14)) >> 15).astype(np.uint8)


def brightness_lut(f):
    return np.clip(_I * float(f), 0, 255).astype(np.uint8)


def contrast_mean(img):
    """The fp64 mean of the grey image: an integer sum over a pixel count."""
    g = grey_u8(img)
    return int(g.astype(np.int64).sum()) / g.size


def contrast_lut(f, mean):
    f = float(f)
    return np.clip(_I * f + mean * (1 - f), 0, 255).astype(np.uint8)


def brightness(img, f):
    return brightness_lut(f)[img]


def contrast(img, f):
    return contrast_lut(f, contrast_mean(img))[img]


def saturation(img, f):
    """cv.addWeighted(img, f, grey, 1 - f, 0) on 8-bit data."""
    f = float(f)
    g = grey_u8(img).astype(F32)[..., None]
    t = img.astype(F32) * F32(f) + g * F32(1 - f)
    assert t.dtype == F32
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def hue(img, f):
    return hsv_shift(img, 180 * float(f), 0.0, 0.0)


def rescale_matrix(scale, h, w):
    alpha, beta = math.cos(0.0) * scale, math.sin(0.0) * scale
    cx, cy = w * 0.5, h * 0.5
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])


_OPS = dict(hsv=hsv_shift, brightness=brightness, contrast=contrast, saturation=saturation, hue=hue,
            lut=lambda img, alpha, beta: R.lut_u8(alpha, beta)[img])


def colour_ops(img, ops):
    """ops: [(name, *parameters)] with name in lut (alpha, beta), hsv (dh, ds, dv), brightness / contrast / saturation /
    hue (factor), applied in order to a uint8 RGB image."""
    for name, *p in ops:
        img = _OPS[name](img, *p)
    return img


def chain(crop, oh, ow, flip=False, ops=(), warps=(), swap=False):
    """warps: forward 2x3 matrices, applied in order (each a cv.warpAffine: uint8 out, zero border)."""
    img = R.resize_linear_u8(crop, (ow, oh))
    if flip:
        img = img[:, ::-1]
    img = colour_ops(np.ascontiguousarray(img), ops)
    for M in warps:
        img = R.warp_affine_u8(np.ascontiguousarray(img), M)
    if swap:
        img = img[..., ::-1]
    return np.ascontiguousarray(img)


def keypoints(kp, h, w, oh, ow, flip=False, warps=(), img_shape=None):
    """kp [9, 2] in crop pixels -> float32 [9, 2]: a scalar fp64 loop over Resize / HorizontalFlip / the warps / ToTensor."""
    out = []
    th, tw = img_shape or (oh, ow)
    for x, y in np.asarray(kp, np.float64):
        x, y = x * (ow / w), y * (oh / h)
        if flip:
            x = (ow - 1) - x
        for M in warps:
            x, y = M[0][0] * x + M[0][1] * y + M[0][2], M[1][0] * x + M[1][1] * y + M[1][2]
        out.append((x, y))
    return (np.asarray(out) / np.asarray([tw, th], np.float32)).astype(np.float32)
