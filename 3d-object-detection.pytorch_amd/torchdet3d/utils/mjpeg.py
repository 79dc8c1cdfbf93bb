"""Motion-JPEG in an AVI 1.0 container, written and read without third-party code: the reference's `cv.VideoWriter` /
`cv.VideoCapture` pair (scripts/demo.py:50-54, 83-84, 112-119) for the one codec this project encodes (`JpegEncoder`) and decodes
(`JpegIndex` / `decode_jpeg_batch`) on the device.  A frame is one complete JPEG file in a `00dc` chunk.

  RIFF 'AVI '
    LIST 'hdrl':  'avih' (56 bytes)   LIST 'strl': 'strh' (56 bytes, 'vids' / 'MJPG'), 'strf' (BITMAPINFOHEADER, 40 bytes)
    LIST 'movi':  '00dc' chunks, each padded to an even length
    'idx1':       16 bytes a frame: '00dc', flags 0x10 (key frame), the chunk's offset from the 'movi' fourcc, its length
"""
import struct
from fractions import Fraction

__all__ = ['MjpegWriter', 'MjpegReader']

_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10
_MOVI_AT = 12 + 12 + 8 + 56 + 12 + 8 + 56 + 8 + 40 + 8         # the file offset of the 'movi' fourcc


class MjpegWriter:
    """`MjpegWriter(path, fps, size)`, size = (width, height) as `cv.VideoWriter` takes it.  `.write(jpeg_bytes)` appends one
    frame (a whole JPEG file of that size); `.close()` writes the index and patches every size and frame count.  A context
    manager.  The RIFF sizes are 32 bits: a file stays below 4 GiB (ValueError from `write` at the limit)."""

    def __init__(self, path, fps, size):
        rate = Fraction(fps).limit_denominator(100000)
        w, h = (int(v) for v in size)
        if rate <= 0 or not 1 <= w <= 65535 or not 1 <= h <= 65535:
            raise ValueError('fps > 0 and size = (width, height) in 1 .. 65535')
        self.rate, self.scale, self.w, self.h = rate.numerator, rate.denominator, w, h
        self.index, self.largest = [], 0
        self.f = open(path, 'wb')
        self.f.write(self._headers(0))
        self.pos = _MOVI_AT + 4

    def _headers(self, movi_bytes):
        n = len(self.index)
        usec = int(round(1e6 * self.scale / self.rate))
        per_sec = int(sum(s for _, s in self.index) * self.rate / (self.scale * n)) if n else 0
        avih = struct.pack('<14I', usec, per_sec, 0, _AVIF_HASINDEX, n, 0, 1, self.largest, self.w, self.h, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIIIHHHH', b'vids', b'MJPG', 0, 0, 0, 0, self.scale, self.rate, 0, n, self.largest,
                           0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.w, self.h, 1, 24, b'MJPG', self.w * self.h * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        riff = 4 + 8 + len(hdrl) + 8 + movi_bytes + 8 + 16 * n
        head = (b'RIFF' + struct.pack('<I', riff) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl
                + b'LIST' + struct.pack('<I', movi_bytes) + b'movi')
        assert len(head) == _MOVI_AT + 4
        return head

    def write(self, jpeg_bytes):
        if self.f is None:
            raise ValueError('the writer is closed')
        data = bytes(jpeg_bytes)
        if self.pos + 8 + len(data) + 1 + 8 + 16 * (len(self.index) + 1) >= 1 << 32:
            raise ValueError('an AVI 1.0 file stays below 4 GiB')
        self.f.write(b'00dc' + struct.pack('<I', len(data)) + data + b'\0' * (len(data) & 1))
        self.index.append((self.pos - _MOVI_AT, len(data)))
        self.largest = max(self.largest, len(data))
        self.pos += 8 + len(data) + (len(data) & 1)

    def close(self):
        if self.f is None:
            return
        self.f.write(b'idx1' + struct.pack('<I', 16 * len(self.index)))
        for off, size in self.index:
            self.f.write(struct.pack('<4sIII', b'00dc', _AVIIF_KEYFRAME, off, size))
        self.f.seek(0)
        self.f.write(self._headers(self.pos - _MOVI_AT))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MjpegReader:
    """`MjpegReader(path)`: iterating yields the `00dc` payloads as `bytes`, in order; `reader[i]` is frame i.  `.fps` (a float),
    `.size` = (width, height) and `len()` come from the headers.  The frames are found through `idx1`; a file without one (a
    recording that was cut off behind its last whole frame) is walked chunk by chunk.  ValueError: not a RIFF AVI file, no
    video stream header, or a chunk that reaches past the end of the file (a truncated file)."""

    def __init__(self, path):
        self.f = open(path, 'rb')
        try:
            self._parse()
        except Exception:
            self.f.close()
            raise

    def _chunk(self, pos, end):
        """The chunk at `pos` inside [.., end) -> (fourcc, payload offset, payload bytes)."""
        if pos + 8 > end:
            raise ValueError(f'truncated AVI file: a chunk header at {pos} reaches past {end}')
        self.f.seek(pos)
        cc, size = struct.unpack('<4sI', self.f.read(8))
        if pos + 8 + size > end:
            raise ValueError(f'truncated AVI file: chunk {cc!r} at {pos} has {size} bytes, {end - pos - 8} are there')
        return cc, pos + 8, size

    def _parse(self):
        self.f.seek(0, 2)
        file_end = self.f.tell()
        self.f.seek(0)
        head = self.f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'AVI ':
            raise ValueError('not a RIFF AVI file')
        avih = strh = strf = movi = idx1 = None
        pos = 12
        while pos + 8 <= file_end:
            cc, at, size = self._chunk(pos, file_end)
            if cc == b'LIST':
                if size < 4:
                    raise ValueError('truncated AVI file: a LIST without a type')
                kind = self.f.read(4)
                if kind == b'hdrl':
                    avih, strh, strf = self._headers(at + 4, at + size)
                elif kind == b'movi' and movi is None:
                    movi = (at, at + size)
            elif cc == b'idx1' and idx1 is None:
                idx1 = (at, size)
            pos = at + size + (size & 1)
        if avih is None or strh is None or strf is None or movi is None:
            raise ValueError('an AVI file needs avih, a video stream (strh, strf) and a movi list')
        self.count = struct.unpack_from('<I', avih, 16)[0]
        scale, rate = struct.unpack_from('<II', strh, 20)
        if strh[:4] != b'vids' or scale == 0 or rate == 0:
            raise ValueError('the first stream is not a video stream with a frame rate')
        self.fps = rate / scale
        w, h = struct.unpack_from('<ii', strf, 4)
        self.size = (w, abs(h))
        self.compression = strf[16:20]
        self.frames = self._from_index(idx1, movi) if idx1 is not None else self._walk(movi)
        if len(self.frames) != self.count:
            raise ValueError(f'the headers promise {self.count} frames, the file holds {len(self.frames)}')

    def _headers(self, pos, end):
        avih = strh = strf = None
        while pos + 8 <= end:
            cc, at, size = self._chunk(pos, end)
            if cc == b'avih' and size >= 40:
                avih = self.f.read(size)
            elif cc == b'LIST' and size >= 4 and self.f.read(4) == b'strl' and strh is None:
                p = at + 4
                while p + 8 <= at + size:
                    c2, a2, s2 = self._chunk(p, at + size)
                    if c2 == b'strh' and s2 >= 48:
                        strh = self.f.read(s2)
                    elif c2 == b'strf' and s2 >= 40:
                        strf = self.f.read(s2)
                    p = a2 + s2 + (s2 & 1)
            pos = at + size + (size & 1)
        return avih, strh, strf

    def _from_index(self, idx1, movi):
        at, size = idx1
        self.f.seek(at)
        raw = self.f.read(size)
        out = []
        for k in range(size // 16):
            cc, _, off, n = struct.unpack_from('<4sIII', raw, 16 * k)
            if cc[2:] not in (b'dc', b'db') or cc[:2] != b'00':
                continue
            pos = movi[0] + off                          # (offsets count from the 'movi' fourcc)
            c2, a2, s2 = self._chunk(pos, movi[1])
            if c2 != cc or s2 != n:
                raise ValueError(f'idx1 entry {k} names a {cc!r} chunk of {n} bytes at {pos}, the file has {c2!r} of {s2}')
            out.append((a2, s2))
        return out

    def _walk(self, movi):
        out, pos = [], movi[0] + 4
        while pos + 8 <= movi[1]:
            cc, at, size = self._chunk(pos, movi[1])
            if cc == b'00dc':
                out.append((at, size))
            pos = at + size + (size & 1)
        return out

    def __len__(self):
        return self.count

    def __getitem__(self, i):
        if self.f is None:
            raise ValueError('the reader is closed')
        at, size = self.frames[i]
        self.f.seek(at)
        return self.f.read(size)

    def __iter__(self):
        return (self[i] for i in range(len(self.frames)))

    def frames_device(self, start, count, device=None):
        """Frames start .. start + count - 1 decoded on the device -> (uint8 [count, H, W, 3], (index status, decode status)): the
        tensor `FramePipeline.process_device` takes, and the two device int32 [count] status vectors of
        `decode_jpeg_frames` (0, 0: decoded).  No host scan walk, nothing read back.  For chunks that are baseline files of the
        stream's size; ValueError for a chunk whose markers the device path does not take or whose size is another (the caller
        has Pillow for those)."""
        from ..dataloaders import jpeg as J
        start, count = int(start), int(count)
        if count < 1 or start < 0 or start + count > len(self.frames):
            raise ValueError(f'frames {start} .. {start + count - 1} of {len(self.frames)}')
        files = [self[i] for i in range(start, start + count)]
        packed, desc = J.decode_jpeg_frames(files, device)
        W, H = self.size
        if not (desc[:, 1] == H).all() or not (desc[:, 2] == W).all():
            raise ValueError(f'a chunk is not {H} x {W}, the size the stream header states')
        return packed.view(count, H, W, 3), J.decode_jpeg_frames.last_status

    def close(self):
        if self.f is not None:
            self.f.close()
            self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
