"""Seeded JPEG test images shared by tests/test_jpeg_host.py, tests/test_jpeg_lane_host.py and tests/test_gpu_jpeg.py: a smooth
field plus noise with a constant 0 block, a constant 255 block and alternating 0 / 255 rows, encoded with Pillow over the matrix
of sizes, samplings and qualities the device decode is pinned on; and the truncations and mutations of one of them."""
import io
import os

import numpy as np
from PIL import Image

# (h, w): 1 x 1, single rows / columns, dw <= 2 (49x2, 7x4: libjpeg replicates instead of its fancy upsampling), ragged MCUs on
# both edges (37x53, 17x33), whole MCUs (16x16), several MCU rows
SIZES = [(1, 1), (1, 7), (2, 40), (3, 6), (5, 3), (7, 4), (8, 9), (9, 5), (16, 16), (17, 33), (33, 17), (37, 53), (49, 2), (24, 40),
         (40, 56)]
SAMPLINGS = ['444', '420', 'gray']
QUALITIES = [(5, False), (35, False), (90, False), (100, False), (100, True), (75, True)]      # (quality, optimize)


def image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 7 + c) + 20 * np.cos(yy / 5 + 2 * c) for c in range(3)], -1) + rng.integers(-20, 21, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[:min(h, 8) // 2, :min(w, 8) // 2] = 0                   # a constant 0 block
    img[h - min(h, 8) // 2:, w - min(w, 8) // 2:] = 255         # a constant 255 block
    if h >= 16:                                                 # alternating 0 / 255 rows
        img[8:16:2, :w // 2], img[9:16:2, :w // 2] = 0, 255
    return img


def encode(img, sampling='420', quality=90, optimize=False, **kw):
    buf = io.BytesIO()
    if sampling == 'gray':
        Image.fromarray(img[..., 0]).save(buf, format='JPEG', quality=quality, optimize=optimize, **kw)
    else:
        Image.fromarray(img).save(buf, format='JPEG', quality=quality, optimize=optimize, subsampling={'444': 0, '422': 1, '420': 2}[sampling],
                                  **kw)
    return buf.getvalue()


_matrix = None


def matrix():
    """[(name, bytes)] over SIZES x SAMPLINGS x QUALITIES (270 files of a few hundred bytes), made once."""
    global _matrix
    if _matrix is None:
        _matrix, n = [], 0
        for h, w in SIZES:
            for s in SAMPLINGS:
                for q, opt in QUALITIES:
                    _matrix.append((f'{h}x{w}_{s}_q{q}_{int(opt)}', encode(image(h, w, n), s, q, opt)))
                    n += 1
    return _matrix


_malformed = None


def malformed():
    """(base, [bytes]): one 17 x 33 4:2:0 file, then every truncation of it (the first len(base) entries) and 200 copies with
    one byte replaced (seeded); made once.  Most are malformed, some mutations still decode."""
    global _malformed
    if _malformed is None:
        base = encode(image(17, 33, 5), '420', 75)
        corpus = [base[:n] for n in range(len(base))]
        rng = np.random.default_rng(11)
        for _ in range(200):
            m = bytearray(base)
            m[int(rng.integers(0, len(base)))] = int(rng.integers(0, 256))
            corpus.append(bytes(m))
        _malformed = (base, corpus)
    return _malformed


def write_files(out, files):
    """Writes [bytes] to out/0000.jpg, 0001.jpg, ... (the directory tools/jpeg_index_check.cpp walks)."""
    os.makedirs(out, exist_ok=True)
    for i, data in enumerate(files):
        with open(os.path.join(out, f'{i:04d}.jpg'), 'wb') as f:
            f.write(data)


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
