"""The baseline JPEG decode of include/t3d.h (next to t3d_jpeg_index), restated literally in numpy: marker parsing, Huffman
decoding bit by bit, jpeg_idct_islow in int32, libjpeg's fancy 4:2:0 upsampling and its YCbCr -> RGB.  This file together with
include/t3d.h is the definition `t3d_jpeg_decode_u8` (csrc/jpeg.hip) is bit-exact against; it equals Pillow on libjpeg-turbo
bit for bit (tests/test_jpeg_host.py).  Slow and plain on purpose: small test images only.

`decode(data)` walks the scan from its first bit.  `decode(data, segs, seg_mcus)` starts every segment afresh from the position
and DC predictors the index gives for it (`segs`: records with fields byte, bit, pred -- what t3d_jpeg_index writes), which is
what the device does, one lane per segment."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
GRAY, S444, S420 = 0, 1, 2


def FIX(x):
    return int(x * 65536 + 0.5)


def parse(data):
    """-> dict(h, w, ncomp, sampling, quant [ncomp][64] natural order, dc / ac: per component {(length, code): symbol},
    scan: offset of the first entropy-coded byte).  Only what the device decode supports; anything else raises ValueError."""
    data = bytes(data)
    if data[:2] != b'\xff\xd8':
        raise ValueError('no SOI')
    qt, huff, frame, pos = {}, {}, None, 2
    while True:
        if data[pos] != 0xFF:
            raise ValueError('no marker')
        while data[pos + 1] == 0xFF:
            pos += 1
        m = data[pos + 1]
        pos += 2
        n = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2:pos + n]
        if m == 0xDB:
            o = 0
            while o < len(seg):
                if seg[o] >> 4:
                    raise ValueError('16-bit quantisation table')
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[o + 1:o + 65], np.uint8)
                qt[seg[o] & 15] = t
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                bits = seg[o + 1:o + 17]
                codes, code, k = {}, 0, o + 17
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        codes[(length, code)] = seg[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[(seg[o] >> 4, seg[o] & 15)] = codes
                o = k
        elif m == 0xC0:
            if seg[0] != 8:
                raise ValueError('precision')
            frame = dict(h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4],
                         comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
        elif 0xC1 <= m <= 0xCF:
            raise ValueError('not a baseline frame')
        elif m == 0xDD:
            if seg[0] or seg[1]:
                raise ValueError('restart interval')
        elif m == 0xDA:
            ns = seg[0]
            if frame is None or ns != len(frame['comps']):
                raise ValueError('more than one scan')
            samp = [(c[1], c[2]) for c in frame['comps']]
            if ns == 1:
                sampling = GRAY
            elif samp == [(1, 1)] * 3:
                sampling = S444
            elif samp == [(2, 2), (1, 1), (1, 1)]:
                sampling = S420
            else:
                raise ValueError('sampling')
            return dict(h=frame['h'], w=frame['w'], ncomp=ns, sampling=sampling, quant=[qt[c[3]] for c in frame['comps']],
                        dc=[huff[(0, seg[2 + 2 * c] >> 4)] for c in range(ns)], ac=[huff[(1, seg[2 + 2 * c] & 15)] for c in range(ns)],
                        scan=pos + n)
        pos += n


class _Bits:
    """The scan as a list of bits, FF 00 unstuffed, zeros behind a marker or the end; `at[offset]`: the index of the first bit
    of the byte at that offset of the STUFFED scan."""

    def __init__(self, scan):
        out, self.at, i = [], {}, 0
        while i < len(scan):
            b = scan[i]
            if b == 0xFF and (i + 1 >= len(scan) or scan[i + 1] != 0):
                break
            self.at[i] = 8 * len(out)
            out.append(b)
            i += 2 if b == 0xFF else 1
        self.end = i                       # offset of the marker behind the scan
        self.real = 8 * len(out)
        self.bits = np.unpackbits(np.array(out, np.uint8)).tolist() + [0] * 64
        self.p = 0

    def bit(self):
        v = self.bits[self.p] if self.p < len(self.bits) else 0
        self.p += 1
        return v

    def get(self, n):
        v = 0
        for _ in range(n):
            v = 2 * v + self.bit()
        return v

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = 2 * code + self.bit()
            s = codes.get((length, code))
            if s is not None:
                return s
        raise ValueError('a code that does not exist')


def extend(v, t):
    return v - (1 << t) + 1 if t and v < (1 << (t - 1)) else v


def coefficients(data, segs=None, seg_mcus=None):
    """-> (parsed, per component int32 [blocks down, blocks across, 64] quantised coefficients in natural order, MCU padding
    included)."""
    p = parse(data)
    f = 2 if p['sampling'] == S420 else 1
    mx, my = -(-p['w'] // (8 * f)), -(-p['h'] // (8 * f))
    fac = [f] + [1] * (p['ncomp'] - 1)
    coef = [np.zeros((my * fc, mx * fc, 64), np.int32) for fc in fac]
    br = _Bits(bytes(data)[p['scan']:])
    pred = [0] * p['ncomp']
    for m in range(mx * my):
        if segs is not None and m % seg_mcus == 0:
            s = segs[m // seg_mcus]
            br.p = br.at[int(s['byte'])] + int(s['bit'])
            pred = [int(v) for v in s['pred'][:p['ncomp']]]
        for c in range(p['ncomp']):
            for b in range(fac[c] * fac[c]):
                blk = coef[c][(m // mx) * fac[c] + b // fac[c], (m % mx) * fac[c] + b % fac[c]]
                t = br.symbol(p['dc'][c])
                pred[c] += extend(br.get(t), t)
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = br.symbol(p['ac'][c])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise ValueError('a run past coefficient 63')
                    blk[ZIGZAG[k]] = extend(br.get(s), s)
                    k += 1
        if br.p > br.real:
            raise ValueError('the scan ends inside an MCU')
    return p, coef


def _idct8(v, shift):
    """jpeg_idct_islow's butterfly along axis 0 of int32 [8, ...], descaled by (x + 2^(shift-1)) >> shift."""
    i32 = np.int32
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * i32(4433)
    tmp2 = z1 + z3 * i32(-15137)
    tmp3 = z1 + z2 * i32(6270)
    z2, z3 = v[0], v[4]
    tmp0 = (z2 + z3) << i32(13)
    tmp1 = (z2 - z3) << i32(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * i32(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * i32(2446), tmp1 * i32(16819), tmp2 * i32(25172), tmp3 * i32(12299)
    z1, z2, z3, z4 = z1 * i32(-7373), z2 * i32(-20995), z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rnd = i32(1 << (shift - 1))
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + rnd) >> i32(shift) for o in out])


def planes(p, coef):
    """Dequantise and inverse-transform every block -> per component uint8 [8 * blocks down, 8 * blocks across]."""
    out = []
    for c, q in zip(coef, p['quant']):
        bh, bw = c.shape[:2]
        ws = (c * q.astype(np.int32)).reshape(bh, bw, 8, 8)                 # [.., row, column]
        ws = _idct8(np.moveaxis(ws, 2, 0), 11)                               # columns: along the rows axis -> [row', bh, bw, column]
        ws = _idct8(np.moveaxis(ws, 3, 0), 18)                               # rows: along the columns axis -> [column', row', bh, bw]
        px = np.clip(ws + np.int32(128), 0, 255).astype(np.uint8)
        out.append(px.transpose(2, 1, 3, 0).reshape(bh * 8, bw * 8))
    return out


def upsample420(s, h, w):
    """One chroma plane (MCU padding included) -> int32 [h, w]: libjpeg's h2v2 fancy upsampling over the dh x dw real samples,
    plain replication when dw <= 2."""
    dh, dw = (h + 1) // 2, (w + 1) // 2
    s = s[:dh, :dw].astype(np.int32)
    if dw <= 2:
        return np.repeat(np.repeat(s, 2, 0), 2, 1)[:h, :w]
    out = np.zeros((2 * dh, 2 * dw), np.int32)
    r = np.arange(dh)
    for v in (0, 1):
        other = np.maximum(r - 1, 0) if v == 0 else np.minimum(r + 1, dh - 1)
        colsum = 3 * s + s[other]
        left = np.concatenate([colsum[:, :1], colsum[:, :-1]], 1)
        right = np.concatenate([colsum[:, 1:], colsum[:, -1:]], 1)
        even, odd = (3 * colsum + left + 8) >> 4, (3 * colsum + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * colsum[:, 0] + 8) >> 4, (4 * colsum[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out[:h, :w]


def decode(data, segs=None, seg_mcus=None):
    """-> uint8 [h, w, 3] RGB, what Image.open(...).convert('RGB') gives on libjpeg-turbo."""
    p, coef = coefficients(data, segs, seg_mcus)
    pl = planes(p, coef)
    h, w = p['h'], p['w']
    y = pl[0][:h, :w].astype(np.int32)
    if p['ncomp'] == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    if p['sampling'] == S420:
        cb, cr = upsample420(pl[1], h, w), upsample420(pl[2], h, w)
    else:
        cb, cr = pl[1][:h, :w].astype(np.int32), pl[2][:h, :w].astype(np.int32)
    cb, cr = cb - 128, cr - 128
    r = y + ((FIX(1.402) * cr + 32768) >> 16)
    g = y + ((-FIX(0.34414) * cb + 32768 - FIX(0.71414) * cr) >> 16)
    b = y + ((FIX(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
