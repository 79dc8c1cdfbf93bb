"""Frames for the JPEG encoder's tests (tests/test_jpeg_encode_host.py, tests/test_gpu_jpeg_encode.py): noise, smooth content, and
six extreme contents -- the cases with ZRL codes, the longest codes and dense FF stuffing.  Pure numpy."""
import io

import numpy as np

SIZES = [(8, 8), (16, 16), (33, 17), (40, 56), (100, 130), (270, 480)]      # three dummy blocks; none; right and bottom; bottom row
QUALITIES = [1, 30, 50, 75, 90, 95, 100]
SAMPLINGS = [2, 1]                      # T3D_JPEG_420, T3D_JPEG_444
EXTREME_SIZE = (24, 40)


def noise(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(y * 3 + x) % 256, (x * 2) % 256, (y + x * 5) // 3 % 256], -1).astype(np.uint8)


def checker(h, w, cell=1):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((((y // cell) + (x // cell)) & 1) * 255).astype(np.uint8)[..., None], 3, 2)


def extremes(h=EXTREME_SIZE[0], w=EXTREME_SIZE[1]):
    """[(name, frame)]: pixel checkerboard, 8x8 block checkerboard, flat, one high-frequency pixel per block, saturated
    primaries, one-pixel column stripes."""
    y, x = np.mgrid[0:h, 0:w]
    flat = np.full((h, w, 3), 137, np.uint8)
    spike = np.full((h, w, 3), 128, np.uint8)
    spike[7::8, 7::8] = (255, 0, 255)
    prim = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)], np.uint8)
    primaries = prim[((y // 3) * 5 + x // 2) % 6]
    stripes = np.repeat(((x & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    return [('pixel checkerboard', checker(h, w)), ('block checkerboard', checker(h, w, 8)), ('flat', flat), ('spike per block', spike),
            ('saturated primaries', primaries), ('column stripes', stripes)]


def pillow(rgb, quality, sampling):
    """The file Pillow writes: Image.save(format='JPEG', quality=q, subsampling=s), optimize and progressive off."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format='JPEG', quality=quality, subsampling={1: 0, 2: 2}[sampling])
    return b.getvalue()


def drawn(h, w, seed=0):
    """Smooth content with drawn rectangles (what an annotated frame looks like)."""
    f = smooth(h, w)
    rng = np.random.default_rng(seed)
    for k in range(6):
        y0, x0 = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
        y1, x1 = min(h, y0 + int(rng.integers(20, h // 2))), min(w, x0 + int(rng.integers(20, w // 2)))
        col = rng.integers(0, 256, 3).astype(np.uint8)
        f[y0:y0 + 3, x0:x1] = col
        f[y1 - 3:y1, x0:x1] = col
        f[y0:y1, x0:x0 + 3] = col
        f[y0:y1, x1 - 3:x1] = col
    return f
