"""CPU: the Motion-JPEG AVI writer and reader (torchdet3d/utils/mjpeg.py).  The container is checked by a RIFF walk of the test's
own -- every chunk and list size, the even padding, the frame counts, rate and scale of avih and strh, the BITMAPINFOHEADER, every
idx1 entry against the 00dc chunk it names -- and the reader returns the written byte strings, with and without idx1."""
import struct

import pytest

from torchdet3d.utils.mjpeg import MjpegReader, MjpegWriter


def _frames(n):
    """n byte strings of odd and even lengths (the container does not look inside them)."""
    return [bytes([0xFF, 0xD8]) + bytes((7 * i + k) & 255 for k in range(101 + 38 * i + (i & 1))) + bytes([0xFF, 0xD9]) for i in range(n)]


def _chunks(b, pos, end):
    """[(fourcc, payload offset, size)] of the chunks in b[pos:end]; every chunk lies inside and the next begins on an even offset."""
    out = []
    while pos < end:
        assert pos + 8 <= end, 'a chunk header past the end of its list'
        cc, size = struct.unpack_from('<4sI', b, pos)
        assert pos + 8 + size <= end, (cc, pos, size, end)
        out.append((cc, pos + 8, size))
        pos += 8 + size + (size & 1)
        if size & 1 and pos <= end:
            assert b[pos - 1] == 0, 'the pad byte'
    assert pos == end or pos == end + 1
    return out


def _walk(b):
    """The whole file -> dict(avih, strh, strf (payloads), movi [(offset of the chunk header, payload)], movi_at, idx1)."""
    assert b[:4] == b'RIFF' and b[8:12] == b'AVI ' and struct.unpack_from('<I', b, 4)[0] == len(b) - 8
    top = _chunks(b, 12, len(b))
    assert [c for c, _, _ in top] == [b'LIST', b'LIST', b'idx1']
    (_, h_at, h_size), (_, m_at, m_size), (_, i_at, i_size) = top
    assert b[h_at:h_at + 4] == b'hdrl' and b[m_at:m_at + 4] == b'movi'
    hdrl = _chunks(b, h_at + 4, h_at + h_size)
    assert [c for c, _, _ in hdrl] == [b'avih', b'LIST']
    assert hdrl[0][2] == 56 and b[hdrl[1][1]:hdrl[1][1] + 4] == b'strl'
    strl = _chunks(b, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [(c, s) for c, _, s in strl] == [(b'strh', 56), (b'strf', 40)]
    movi = _chunks(b, m_at + 4, m_at + m_size)
    assert all(c == b'00dc' for c, _, _ in movi)
    return dict(avih=b[hdrl[0][1]:hdrl[0][1] + 56], strh=b[strl[0][1]:strl[0][1] + 56], strf=b[strl[1][1]:strl[1][1] + 40],
                movi=[(at - 8, b[at:at + size]) for _, at, size in movi], movi_at=m_at, idx1=b[i_at:i_at + i_size])


@pytest.mark.parametrize('n', [0, 1, 5])
def test_container_walk(tmp_path, n):
    path, frames = str(tmp_path / 'v.avi'), _frames(n)
    with MjpegWriter(path, 30000 / 1001, (480, 270)) as wr:
        for f in frames:
            wr.write(f)
    b = open(path, 'rb').read()
    w = _walk(b)
    assert [p for _, p in w['movi']] == frames
    assert n == 0 or len(frames[0]) & 1 and (n == 1 or not len(frames[1]) & 1), 'odd and even lengths'
    usec, _, _, flags, total, _, streams, largest, width, height = struct.unpack_from('<10I', w['avih'])
    assert (usec, flags & 0x10, total, streams, width, height) == (33367, 0x10, n, 1, 480, 270)
    assert largest == max([len(f) for f in frames] + [0])
    kind, handler = struct.unpack_from('<4s4s', w['strh'])
    scale, rate, start, length = struct.unpack_from('<4I', w['strh'], 20)
    assert (kind, handler, scale, rate, start, length) == (b'vids', b'MJPG', 1001, 30000, 0, n)
    assert struct.unpack_from('<4H', w['strh'], 48) == (0, 0, 480, 270)
    size, bw, bh, planes, bits, comp, image = struct.unpack_from('<IiiHH4sI', w['strf'])
    assert (size, bw, bh, planes, bits, comp, image) == (40, 480, 270, 1, 24, b'MJPG', 480 * 270 * 3)
    assert len(w['idx1']) == 16 * n
    for k, (at, payload) in enumerate(w['movi']):
        cc, flags, off, length = struct.unpack_from('<4sIII', w['idx1'], 16 * k)
        assert (cc, flags, length) == (b'00dc', 0x10, len(payload))
        assert w['movi_at'] + off == at, 'idx1 offsets count from the movi fourcc'
        assert b[at:at + 8] == b'00dc' + struct.pack('<I', length)


def test_integer_rate_and_closed_writer(tmp_path):
    path = str(tmp_path / 'v.avi')
    wr = MjpegWriter(path, 25, (16, 8))
    wr.write(b'\xff\xd8\xff\xd9')
    wr.close()
    wr.close()
    with pytest.raises(ValueError):
        wr.write(b'x')
    scale, rate = struct.unpack_from('<2I', _walk(open(path, 'rb').read())['strh'], 20)
    assert (scale, rate) == (1, 25)
    for fps, size in ((0, (16, 8)), (25, (0, 8)), (25, (16, 70000))):
        with pytest.raises(ValueError):
            MjpegWriter(str(tmp_path / 'bad.avi'), fps, size)


@pytest.mark.parametrize('n', [0, 1, 5])
def test_reader_returns_the_written_frames_with_and_without_idx1(tmp_path, n):
    path, cut, frames = str(tmp_path / 'v.avi'), str(tmp_path / 'cut.avi'), _frames(n)
    with MjpegWriter(path, 30, (480, 270)) as wr:
        for f in frames:
            wr.write(f)
    b = open(path, 'rb').read()
    open(cut, 'wb').write(b[:len(b) - 8 - 16 * n])        # the idx1 chunk cut off
    for p in (path, cut):
        with MjpegReader(p) as rd:
            assert (rd.fps, rd.size, len(rd)) == (30.0, (480, 270), n)
            assert list(rd) == frames
            assert [rd[i] for i in range(n)] == frames
            assert rd.compression == b'MJPG'


def test_reader_refuses_truncated_and_foreign_files(tmp_path):
    path, frames = str(tmp_path / 'v.avi'), _frames(5)
    with MjpegWriter(path, 30, (480, 270)) as wr:
        for f in frames:
            wr.write(f)
    b = open(path, 'rb').read()
    movi_end = len(b) - 8 - 16 * 5
    bad = str(tmp_path / 'bad.avi')
    for n in (movi_end - 1, movi_end - 200, 224 + 50, 224, 100, 11, len(b) - 3, len(b) - 16 * 5 + 1):
        open(bad, 'wb').write(b[:n])
        with pytest.raises(ValueError):
            MjpegReader(bad)
    open(bad, 'wb').write(b'RIFF' + b[4:8] + b'WAVE' + b[12:])
    with pytest.raises(ValueError):
        MjpegReader(bad)
    wrong = bytearray(b)
    struct.pack_into('<I', wrong, len(b) - 16 * 4 + 8, 6)          # an idx1 entry that points into the middle of a frame
    open(bad, 'wb').write(bytes(wrong))
    with pytest.raises(ValueError):
        MjpegReader(bad)
