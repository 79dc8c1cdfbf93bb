"""Baseline JPEG encode on the device (include/t3d.h next to t3d_jpeg_encode_setup; csrc/jpeg_encode.h, csrc/jpeg_encode.hip):
the output side of the demo chain.  The reference ends each frame in `vout.write(vis)` (scripts/demo.py:50-54, 83-84); here
the frames `FramePipeline.process_device` drew on stay on the device, `JpegEncoder.encode_device` turns them into JPEG files
there, and only the files' bytes are read back (`encode`) -- for `MjpegWriter` (utils/mjpeg.py), a socket, or a disk.

The files are Pillow-on-libjpeg-turbo's `Image.save(format='JPEG', quality=q, subsampling=s)` byte for byte (pinned by the
tests), carry no restart markers and so are the kind `t3d_jpeg_index` / `t3d_jpeg_decode_u8` take back."""
import ctypes

import numpy as np
import torch

from .. import _native as N

__all__ = ['JpegEncoder', 'encode_tables', 'ENC_TABLES_DTYPE', 'ENC_RESULT_DTYPE', 'DEFAULT_ENC_SEG_MCUS', 'SAMPLINGS']

# include/t3d.h: t3d_jpeg_enc_tables (5040 bytes) and t3d_jpeg_enc_result (16); csrc/jpeg_encode.hip asserts the same offsets
ENC_TABLES_DTYPE = np.dtype([('h', '<i4'), ('w', '<i4'), ('quality', '<i4'), ('sampling', '<i4'), ('mcus_x', '<i4'), ('mcus_y', '<i4'),
                             ('mcu_blocks', '<i4'), ('blocks', '<i4'), ('luma_rows', '<i4'), ('luma_cols', '<i4'),
                             ('header_bytes', '<i4'), ('reserved', '<i4'), ('divisor', '<u2', (2, 64)), ('huff', '<u4', (4, 256)),
                             ('header', 'u1', (640,))])
ENC_RESULT_DTYPE = np.dtype([('bytes', '<i8'), ('overflow', '<i4'), ('reserved', '<i4')])
assert ENC_TABLES_DTYPE.itemsize == 5040 and ENC_RESULT_DTYPE.itemsize == 16
# MCUs per segment = per entropy lane.  tools/time_jpeg_encode.py sweeps 1 .. 16: the best of the sweep,
# at one frame and at eight -- the walk of a segment is serial, so the shortest segment has the most lanes
DEFAULT_ENC_SEG_MCUS = 1
SAMPLINGS = {'444': 1, '420': 2}        # include/t3d.h: T3D_JPEG_444 / T3D_JPEG_420


def encode_tables(h, w, quality=90, sampling='420'):
    """-> (return code of t3d_jpeg_encode_setup, the filled ENC_TABLES_DTYPE record as an array of one).  Host only: no GPU is
    touched.  sampling: '444' / '420' or the T3D_JPEG_* code."""
    t = np.zeros(1, ENC_TABLES_DTYPE)
    code = SAMPLINGS.get(sampling, sampling) if isinstance(sampling, str) else sampling
    if isinstance(code, str):
        return N.ERR_ARG, t
    return N.lib().t3d_jpeg_encode_setup(int(h), int(w), int(quality), int(code), t.ctypes.data), t


class JpegEncoder:
    """`JpegEncoder(h, w, quality=90, sampling='420', max_frames=1, cap_bytes=None, seg_mcus=None, device=None)`: up to
    `max_frames` RGB frames of h x w a call.  cap_bytes: a file's slot in the output (default h * w * 3); a frame whose file does
    not fit is flagged, `encode` then encodes it again with a slot that does.  An encoder's calls share its output and work
    buffers: calls on different streams are the caller's to order (as for any tensor used on two streams)."""

    def __init__(self, h, w, quality=90, sampling='420', max_frames=1, cap_bytes=None, seg_mcus=None, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError('the JPEG encoder runs on the GPU (no CPU fallback)')
        rc, self.tables = encode_tables(h, w, quality, sampling)
        if rc != 0:
            raise ValueError(f'h, w in 1 .. 65535, quality in 1 .. 100, sampling 444 or 420 (got {h}, {w}, {quality}, {sampling!r})')
        self.h, self.w, self.quality, self.sampling = int(h), int(w), int(quality), int(self.tables['sampling'][0])
        self.max_frames = int(max_frames)
        self.seg_mcus = DEFAULT_ENC_SEG_MCUS if seg_mcus is None else int(seg_mcus)
        self.header_bytes = int(self.tables['header_bytes'][0])
        self.cap_bytes = max(self.h * self.w * 3, self.header_bytes + 2) if cap_bytes is None else int(cap_bytes)
        if self.max_frames < 1 or self.max_frames > 65535 or self.seg_mcus < 1 or self.cap_bytes < self.header_bytes + 2:
            raise ValueError('max_frames in 1 .. 65535, seg_mcus >= 1, cap_bytes at least the header + 2')
        dev = torch.device('cuda' if device is None else device)
        self.device = torch.device('cuda', torch.cuda.current_device() if dev.index is None else dev.index)
        self._tables_dev = torch.from_numpy(self.tables.view(np.uint8).copy()).to(self.device)
        self._buffers = {}

    def _for_cap(self, cap):
        """(out, results, work) of a call with slots of `cap` bytes; those of the encoder's own cap_bytes are kept."""
        if cap in self._buffers:
            return self._buffers[cap]
        nbytes = ctypes.c_longlong(0)
        rc = N.lib().t3d_jpeg_encode_work_bytes(self.max_frames, self.h, self.w, self.sampling, self.seg_mcus, cap, ctypes.byref(nbytes))
        if rc != 0:
            raise ValueError(f'cap_bytes = {cap}: at least the header + 2 = {self.header_bytes + 2}')
        bufs = (torch.empty(self.max_frames * cap, dtype=torch.uint8, device=self.device),
                torch.zeros(self.max_frames * 16, dtype=torch.uint8, device=self.device),
                torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=self.device))
        if cap == self.cap_bytes:
            self._buffers[cap] = bufs
        return bufs

    def _checked(self, frames):
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or not frames.is_cuda:
            raise ValueError('frames must be a uint8 device tensor')
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.h, self.w, 3) or not frames.is_contiguous():
            raise ValueError(f'frames must be contiguous [B, {self.h}, {self.w}, 3] or [{self.h}, {self.w}, 3]')
        if frames.shape[0] > self.max_frames:
            raise ValueError(f'{frames.shape[0]} frames for an encoder of max_frames = {self.max_frames}')
        if frames.device != self.device:
            raise ValueError(f'frames on {frames.device}, the encoder on {self.device}')
        return frames

    def encode_device(self, frames, cap_bytes=None):
        """frames uint8 [B, h, w, 3] (or [h, w, 3]) on the device -> (out uint8 [B, cap_bytes], results uint8 [B, 16] holding
        ENC_RESULT_DTYPE rows), device views valid until the next call.  One t3d_jpeg_encode_u8 on the
        current stream; never synchronises."""
        frames = self._checked(frames)
        cap = self.cap_bytes if cap_bytes is None else int(cap_bytes)
        B = frames.shape[0]
        out, results, work = self._for_cap(cap)
        N.call('t3d_jpeg_encode_u8', N.ptr(frames), B, self.tables.ctypes.data, N.ptr(self._tables_dev), self.seg_mcus, N.ptr(out), cap,
               N.ptr(results), N.ptr(work), work.numel(), N.stream())
        return out.view(self.max_frames, cap)[:B], results.view(self.max_frames, 16)[:B]

    def encode(self, frames):
        """-> the B files, a list of `bytes`.  One read-back of the result rows, then one copy of the used bytes; the frames
        flagged `overflow` are encoded once more with slots of twice the reported bytes, which always suffice."""
        frames = self._checked(frames)
        out, results = self.encode_device(frames)
        res = results.cpu().numpy().view(ENC_RESULT_DTYPE).reshape(-1)
        ok = res['overflow'] == 0
        used = int(res['bytes'][ok].max()) if ok.any() else 0
        host = out[:, :used].cpu().numpy() if used else None
        files = [host[i, :int(res['bytes'][i])].tobytes() if ok[i] else None for i in range(len(res))]
        again = np.nonzero(~ok)[0]
        if len(again):
            cap = -(-2 * int(res['bytes'][again].max()) // 64) * 64
            out2, results2 = self.encode_device(frames[torch.from_numpy(again).to(frames.device)].contiguous(), cap_bytes=cap)
            res2 = results2.cpu().numpy().view(ENC_RESULT_DTYPE).reshape(-1)
            if res2['overflow'].any():
                raise RuntimeError('a frame does not fit a slot of twice its unstuffed size')
            host2 = out2[:, :int(res2['bytes'].max())].cpu().numpy()
            for k, i in enumerate(again):
                files[i] = host2[k, :int(res2['bytes'][k])].tobytes()
        return files
