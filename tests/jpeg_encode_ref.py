"""numpy restatement of the device JPEG ENCODER's definition (include/t3d.h next to t3d_jpeg_encode_setup): libjpeg-turbo's
default compression path as Pillow drives it -- `Image.save(format='JPEG', quality=q, subsampling=s)`, optimize and progressive
off -- for RGB uint8 frames, 4:2:0 or 4:4:4.  `encode(rgb, quality, sampling)` returns the WHOLE file; Pillow on libjpeg-turbo
writes the same bytes (tests/test_jpeg_encode_host.py), and so does t3d_jpeg_encode_u8 (tests/test_gpu_jpeg_encode.py).

Pure Python / numpy; imports nothing from the package."""
import numpy as np

S444, S420 = 1, 2                       # include/t3d.h: T3D_JPEG_444 / T3D_JPEG_420

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

# ITU-T T.81 Annex K: the example quantisation tables (natural order) and the typical Huffman tables
K_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (list(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546'
    '4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8'
    'b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')), list(bytes.fromhex(
        '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344'
        '45464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4'
        'b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')))


def quant_tables(quality):
    """-> (luma, chroma) int [64] in natural order: jpeg_set_quality's scaling of the Annex K tables, baseline-clipped."""
    if not 1 <= quality <= 100:
        raise ValueError('quality is 1 .. 100')
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (K_LUMA, K_CHROMA))


def huff_codes(bits, vals):
    """-> (code, length) int [256] by symbol (length 0: the table has no such symbol): the canonical codes of a DHT table."""
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]], size[vals[k]] = c, l
            c, k = c + 1, k + 1
        c <<= 1
    return code, size


def header(h, w, quality, sampling):
    """The bytes in front of the scan: SOI, APP0 (JFIF 1.01, no density unit, 1:1), two DQT, SOF0, four DHT, SOS."""
    out = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for i, q in enumerate(quant_tables(quality)):
        out += b'\xff\xdb\x00\x43' + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    out += b'\xff\xc0\x00\x11\x08' + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22 if sampling == S420 else 0x11, 0,
                                            2, 0x11, 1, 3, 0x11, 1])
    for cls, bits, vals in ((0x00, DC_BITS[0], DC_VALS[0]), (0x10, AC_BITS[0], AC_VALS[0]), (0x01, DC_BITS[1], DC_VALS[1]),
                            (0x11, AC_BITS[1], AC_VALS[1])):
        out += b'\xff\xc4' + bytes([0, 19 + len(vals), cls]) + bytes(bits) + bytes(vals)
    out += b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    return bytes(out)


def _fix(x, bits):
    return int(x * (1 << bits) + 0.5)


def ycc(rgb):
    """jccolor.c, 16 fractional bits -> Y, Cb, Cr int64 [h, w]."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    f = lambda x: _fix(x, 16)
    y = (f(.299) * r + f(.587) * g + f(.114) * b + 32768) >> 16
    cb = (-f(.16874) * r - f(.33126) * g + f(.5) * b + (128 << 16) + 32767) >> 16
    cr = (f(.5) * r - f(.41869) * g - f(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    """Replicate the last row and the last column of p up to rows x cols."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode='edge')


def planes(rgb, sampling):
    """-> [(samples int64 [8 * bh, 8 * bw], real block rows, real block columns)] of Y, Cb, Cr with the edge rules applied; a
    block outside the real rows / columns is a dummy block (4:2:0 luma only) whose samples are not looked at."""
    h, w = rgb.shape[:2]
    y, cb, cr = ycc(rgb)
    up = lambda v, m: -(-v // m) * m
    if sampling == S444:
        return [(_pad(p, up(h, 8), up(w, 8)), up(h, 8) // 8, up(w, 8) // 8) for p in (y, cb, cr)]
    out = [(_pad(_pad(y, up(h, 8), up(w, 8)), up(h, 16), up(w, 16)), up(h, 8) // 8, up(w, 8) // 8)]
    for p in (cb, cr):
        p = _pad(p, up(h, 2), up(w, 16))                # columns to the MCU, rows only to an even count
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        bias = np.where(np.arange(s.shape[1]) & 1, 2, 1)
        s = (s + bias[None, :]) >> 2
        s = _pad(s, up(h, 16) // 2, s.shape[1])         # the last DOWNSAMPLED row, down to the MCU
        out.append((s, s.shape[0] // 8, s.shape[1] // 8))
    return out


_C = {n: _fix(v, 13) for n, v in dict(c0298=0.298631336, c0390=0.390180644, c0541=0.541196100, c0765=0.765366865,
                                      c0899=0.899976223, c1175=1.175875602, c1501=1.501321110, c1847=1.847759065,
                                      c1961=1.961570560, c2053=2.053119869, c2562=2.562915447, c3072=3.072711026).items()}


def _fdct_pass(d, first):
    """jfdctint.c: one pass over the LAST axis of d int64 [..., 8]."""
    ds = lambda x, n: (x + (1 << (n - 1))) >> n
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    n = 11 if first else 15
    o[0] = (t10 + t11) << 2 if first else ds(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else ds(t10 - t11, 2)
    z1 = (t12 + t13) * _C['c0541']
    o[2] = ds(z1 + t13 * _C['c0765'], n)
    o[6] = ds(z1 - t12 * _C['c1847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _C['c1175']
    t4, t5, t6, t7 = t4 * _C['c0298'], t5 * _C['c2053'], t6 * _C['c3072'], t7 * _C['c1501']
    z1, z2, z3, z4 = -z1 * _C['c0899'], -z2 * _C['c2562'], -z3 * _C['c1961'] + z5, -z4 * _C['c0390'] + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_quant(p, q):
    """p int64 [8 * bh, 8 * bw] samples, q int [64] natural order -> quantised coefficients int64 [bh, bw, 64], natural order."""
    bh, bw = p.shape[0] // 8, p.shape[1] // 8
    d = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128          # [bh, bw, row, col]
    d = _fdct_pass(d, True)                                          # along the rows
    d = _fdct_pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)       # along the columns
    c = d.reshape(bh, bw, 64)
    div = 8 * np.asarray(q, np.int64)
    return np.sign(c) * ((np.abs(c) + div // 2) // div)


def coefficients(rgb, quality, sampling):
    """-> int64 [blocks in scan order, 64 in zigzag order]: what the entropy coder is given, dummy blocks included."""
    ql, qc = quant_tables(quality)
    pl = planes(np.asarray(rgb), sampling)
    comps = [fdct_quant(p, q)[..., ZIGZAG] for (p, _, _), q in zip(pl, (ql, qc, qc))]
    my, mx = comps[1].shape[:2]
    if sampling == S444:
        return np.stack(comps, 2).reshape(-1, 64)
    yc, (_, rows, cols) = comps[0], pl[0]
    # dummy luma blocks: no AC; the DC of the block before it in the MCU (right: the left neighbour; bottom: the last of the
    # row above -- itself a dummy where the column is missing too)
    yc = yc.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64).copy()
    for by in range(my):
        for bx in range(mx):
            for b in range(4):
                if 2 * by + (b >> 1) >= rows or 2 * bx + (b & 1) >= cols:
                    yc[by, bx, b, :] = 0
                    yc[by, bx, b, 0] = yc[by, bx, b - 1, 0]
    return np.concatenate([yc, comps[1][:, :, None], comps[2][:, :, None]], 2).reshape(-1, 64)


def _nbits(v):
    v = np.abs(v)
    n = np.zeros(v.shape, np.int64)
    for k in range(16):
        n += (v >> k) > 0
    return n


def scan_bits(coef, sampling):
    """coef [blocks, 64] (scan order, zigzag) -> uint8 array of the scan's BITS, MSB first, before padding and stuffing."""
    bpm = 6 if sampling == S420 else 3
    nblk = coef.shape[0]
    comp = np.tile(np.array([0, 0, 0, 0, 1, 2] if bpm == 6 else [0, 1, 2]), nblk // bpm)
    tab = np.minimum(comp, 1)
    dcc = [huff_codes(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
    acc = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
    dc_code, dc_size = np.stack([c[0] for c in dcc]), np.stack([c[1] for c in dcc])
    ac_code, ac_size = np.stack([c[0] for c in acc]), np.stack([c[1] for c in acc])
    # events [block, slot] = (value, bit count): slot 0 the DC, 4 per AC position (three ZRL, the code with its extra bits), EOB
    val = np.zeros((nblk, 2 + 63 * 4), np.int64)
    cnt = np.zeros((nblk, 2 + 63 * 4), np.int64)
    diff = coef[:, 0].copy()
    for c in range(3):
        i = np.nonzero(comp == c)[0]
        diff[i[1:]] = coef[i[1:], 0] - coef[i[:-1], 0]
    n = _nbits(diff)
    extra = np.where(diff < 0, diff - 1, diff) & ((1 << n) - 1)
    val[:, 0] = (dc_code[tab, n] << n) | extra
    cnt[:, 0] = dc_size[tab, n] + n
    ac = coef[:, 1:]
    nz = ac != 0
    pos = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, pos, 0), 1)            # position of the last non-zero up to here
    prev = np.concatenate([np.zeros((nblk, 1), np.int64), last[:, :-1]], 1)
    run = pos - prev - 1
    n = _nbits(ac)
    extra = np.where(ac < 0, ac - 1, ac) & ((1 << n) - 1)
    sym = ((run & 15) << 4) | n
    t2 = tab[:, None]
    for z in range(3):
        on = nz & ((run >> 4) > z)
        val[:, 1 + z:1 + 63 * 4:4] = np.where(on, ac_code[t2, 0xF0], 0)
        cnt[:, 1 + z:1 + 63 * 4:4] = np.where(on, ac_size[t2, 0xF0], 0)
    val[:, 4:1 + 63 * 4:4] = np.where(nz, (ac_code[t2, sym] << n) | extra, 0)
    cnt[:, 4:1 + 63 * 4:4] = np.where(nz, ac_size[t2, sym] + n, 0)
    eob = last[:, -1] < 63
    val[:, -1] = np.where(eob, ac_code[tab, 0], 0)
    cnt[:, -1] = np.where(eob, ac_size[tab, 0], 0)
    keep = cnt.reshape(-1) > 0
    val, cnt = val.reshape(-1)[keep], cnt.reshape(-1)[keep]
    start = np.cumsum(cnt) - cnt
    owner = np.repeat(np.arange(len(cnt)), cnt)
    j = np.arange(int(cnt.sum())) - start[owner]
    return ((val[owner] >> (cnt[owner] - 1 - j)) & 1).astype(np.uint8)


def scan_bytes(bits):
    """Pad the last byte with 1 bits, then a 00 behind every FF."""
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    b = np.packbits(bits)
    return np.insert(b, np.nonzero(b == 0xFF)[0] + 1, 0).tobytes()


def unstuffed_scan_bytes(rgb, quality=90, sampling=S420):
    """Bytes of the scan before stuffing (the padded last byte included)."""
    return (len(scan_bits(coefficients(rgb, quality, sampling), sampling)) + 7) // 8


def encode(rgb, quality=90, sampling=S420):
    """rgb uint8 [h, w, 3] -> the JPEG file, bytes."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or sampling not in (S444, S420):
        raise ValueError('an RGB uint8 [h, w, 3] frame, 4:4:4 or 4:2:0')
    h, w = rgb.shape[:2]
    return header(h, w, quality, sampling) + scan_bytes(scan_bits(coefficients(rgb, quality, sampling), sampling)) + b'\xff\xd9'
