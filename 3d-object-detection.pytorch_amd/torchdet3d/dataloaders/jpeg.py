"""JPEG frames decoded on the device from a per-file MCU index (include/t3d.h next to t3d_jpeg_index; csrc/jpeg_index.h,
csrc/jpeg.hip).

Baseline Huffman decoding is serial inside a scan and Objectron frames carry no restart markers, so the work is split the way
the crop cache splits the regression loader's: ONCE PER FILE `JpegIndex.build` walks every scan on the host (a thread pool in
the main process -- ctypes releases the GIL; no DataLoader worker ever loads the library) and records where every
`seg_mcus`-th MCU starts; EVERY EPOCH the workers only read file bytes and `t3d_jpeg_decode_u8` decodes all segments of all
frames of a batch in parallel into the packed frame buffer `t3d_detect_augment_u8` reads (`GpuDetectionLoader`,
`ObjectronFrames(decode='device')`).  The pixels are those of Pillow on libjpeg-turbo, bit for bit.

A file the device path does not take (progressive, restart markers, 4:2:2, CMYK, ... or malformed) keeps its reason in the
index and is decoded on the host as before.

The regression loader cuts one object's box out of each frame; the form for it decodes only that pixel RECTANGLE:
`plan_roi` works out, on the host and in numpy, which MCUs the rectangle's pixels read, which segments own them and which bytes
of the file those segments lie in; only that byte span has to be read and uploaded, and `t3d_jpeg_decode_roi_u8`
(`launch_decode_roi`, `decode_jpeg_rois`) writes the packed crops `collate_crops` packs from host-decoded frames.

`decode_jpeg_batch(files, rows)` is the one-call form: a list of file contents and their index rows -> the packed device
buffer and its descriptor table, the layout `collate_frames` produces.

A frame nobody has indexed -- a video or camera frame -- needs no host walk: `read_jpeg_header` reads its markers,
`index_jpeg_device` builds the index rows of a batch on the device (`t3d_jpeg_index_device`: the host indexer's rows, byte for
byte), `decode_jpeg_frames(files)` chains the decode behind it with nothing read back, and `JpegIndex.build(where='device')`
builds a saved index that way."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .staging import pack

__all__ = ['JpegIndex', 'decode_jpeg_batch', 'index_jpeg', 'collate_jpeg', 'INFO_DTYPE', 'SEG_DTYPE', 'ITEM_DTYPE',
           'DEFAULT_SEG_MCUS', 'REASONS', 'roi_mcus', 'plan_roi', 'plan_roi_batch', 'launch_decode_roi', 'decode_jpeg_rois',
           'ROI_SEG_MCUS', 'ROI_READ_AHEAD', 'read_jpeg_header', 'index_jpeg_device', 'decode_jpeg_frames', 'DEFAULT_SUB_BYTES',
           'SUB_BYTES_RANGE', 'launch_decode', 'starts', 'mcu_blocks', 'frame_blocks', 'item_table']

# include/t3d.h: t3d_jpeg_info (864 bytes), t3d_jpeg_seg (16), t3d_jpeg_item (48)
INFO_DTYPE = np.dtype([('h', '<i4'), ('w', '<i4'), ('ncomp', '<i4'), ('sampling', '<i4'), ('mcus_x', '<i4'), ('mcus_y', '<i4'),
                       ('seg_mcus', '<i4'), ('nseg', '<i4'), ('scan_offset', '<i8'), ('scan_bytes', '<i8'), ('reason', '<i4'),
                       ('reserved', '<i4'), ('comp_dc', 'u1', (4,)), ('comp_ac', 'u1', (4,)), ('quant', 'u1', (3, 64)),
                       ('dc_bits', 'u1', (2, 16)), ('dc_vals', 'u1', (2, 16)), ('ac_bits', 'u1', (2, 16)), ('ac_vals', 'u1', (2, 256))])
SEG_DTYPE = np.dtype([('byte', '<u4'), ('pred', '<i2', (3,)), ('bit', 'u1'), ('reserved', 'u1'), ('mcu', '<i4')])
ITEM_DTYPE = np.dtype([('file_offset', '<i8'), ('file_bytes', '<i8'), ('out_offset', '<i8'), ('block_offset', '<i8'),
                       ('seg_offset', '<i8'), ('reserved', '<i8')])
assert INFO_DTYPE.itemsize == 864 and SEG_DTYPE.itemsize == 16 and ITEM_DTYPE.itemsize == 48
# MCUs per segment = per device lane.  tools/time_jpeg_decode.py sweeps 2 .. 120: the best of the sweep
DEFAULT_SEG_MCUS = 2
# why a file stays on the host decode: T3D_JPEG_REASON_* of include/t3d.h, and -1 for a file the indexer calls malformed
REASONS = {0: 'decoded on the device', 1: 'not a baseline frame (progressive, extended, lossless or arithmetic)',
           2: 'sample precision other than 8 bit', 3: 'restart interval', 4: 'sampling other than 4:4:4 / 4:2:0',
           5: 'component count other than 1 or 3', 6: 'more than one scan', 7: '16-bit quantisation table',
           8: 'three components that are not YCbCr', -1: 'malformed'}
# the same for an index made for the rectangle decode: tools/time_roi_decode.py sweeps 1 .. 16: the best
# of the sweep
ROI_SEG_MCUS = 1
# bytes uploaded behind the byte the segment after the last needed one begins in: the device's 64-bit window reads ahead
ROI_READ_AHEAD = 8
# raw bytes of the stuffed scan per lane of the device indexer (include/t3d.h: t3d_jpeg_index_device).  tools/time_jpeg_index.py
# sweeps 4 .. 512: the best of the sweep at 80 frames of 1440 x 1920 (and at 1 and 8 of 1080 x 1920)
DEFAULT_SUB_BYTES = 512
SUB_BYTES_RANGE = (4, 1 << 30)
_INDEX_BATCH = 64                       # files per device call of JpegIndex.build(where='device')
_BLOCKS_PER_MCU = (1, 3, 6)             # gray, 4:4:4, 4:2:0
_MAGIC = 0x7833644A50454731             # 'x3dJPEG1'


def index_jpeg(data, seg_mcus=DEFAULT_SEG_MCUS):
    """One file's bytes -> (return code of t3d_jpeg_index, info record, segment table).  Host only: no GPU is touched."""
    from .. import _native as N
    lib = N.lib()
    a = np.frombuffer(data, np.uint8)
    info = np.zeros(1, INFO_DTYPE)
    rc = lib.t3d_jpeg_index(a.ctypes.data, a.size, int(seg_mcus), info.ctypes.data, None, 0)
    segs = np.zeros(int(info['nseg'][0]) if rc == 0 else 0, SEG_DTYPE)
    if rc == 0:
        rc = lib.t3d_jpeg_index(a.ctypes.data, a.size, int(seg_mcus), info.ctypes.data, segs.ctypes.data, len(segs))
    return rc, info[0], segs


def read_jpeg_header(data, seg_mcus=DEFAULT_SEG_MCUS):
    """One file's bytes -> (return code of t3d_jpeg_header, info record): the markers only, nothing of the scan; the record is
    `index_jpeg`'s except that scan_bytes is the bytes from scan_offset to the file's end.  Host only: no GPU is touched."""
    from .. import _native as N
    a = np.frombuffer(data, np.uint8)
    info = np.zeros(1, INFO_DTYPE)
    rc = N.lib().t3d_jpeg_header(a.ctypes.data, a.size, int(seg_mcus), info.ctypes.data)
    return rc, info[0]


def _reason(rc, info):
    """The return code of t3d_jpeg_index / t3d_jpeg_header and the record it filled -> the key of REASONS."""
    from .. import _native as N
    return 0 if rc == 0 else (int(info['reason']) if rc == N.ERR_UNSUPPORTED else -1)


def starts(counts):
    """counts [n] -> int64 [n]: where each begins when they lie one behind the other."""
    counts = np.asarray(counts, np.int64)
    return np.cumsum(counts) - counts


def mcu_blocks(sampling):
    """8x8 blocks of one MCU, by T3D_JPEG_GRAY / _444 / _420 (a record the device does not decode may hold any value)."""
    return np.asarray(_BLOCKS_PER_MCU, np.int64)[np.clip(sampling, 0, 2)]


def frame_blocks(infos):
    """INFO_DTYPE records -> int64: the 8x8 blocks of each whole frame."""
    return infos['mcus_x'].astype(np.int64) * infos['mcus_y'] * mcu_blocks(infos['sampling'])


def item_table(file_offset, file_bytes, out_offset, seg_offset, blocks):
    """The t3d_jpeg_item table of one call: where each file's bytes, frame and segment rows lie, and `block_offset`, the
    prefix sums of `blocks` (the decode's 8x8 blocks, the device indexer's subsequence records)."""
    items = np.zeros(len(blocks), ITEM_DTYPE)
    items['file_offset'], items['file_bytes'], items['out_offset'] = file_offset, file_bytes, out_offset
    items['seg_offset'], items['block_offset'] = seg_offset, starts(blocks)
    return items


class JpegIndex:
    """The index of a list of files, as flat numpy arrays: `infos` [n] INFO_DTYPE, `segs` [total] SEG_DTYPE, `seg_start` int64
    [n + 1] (file i owns segs[seg_start[i]:seg_start[i + 1]]), `size` and `mtime_ns` int64 [n] of the file when it was indexed,
    `reason` int64 [n] (0: the device decodes it; REASONS), `files` (the names, relative to the root)."""

    def __init__(self, files, infos, segs, seg_start, size, mtime_ns, reason, seg_mcus):
        self.files, self.infos, self.segs, self.seg_start = list(files), infos, segs, seg_start
        self.size, self.mtime_ns, self.reason, self.seg_mcus = size, mtime_ns, reason, int(seg_mcus)

    def __len__(self):
        return len(self.files)

    @classmethod
    def build(cls, files, root, seg_mcus=DEFAULT_SEG_MCUS, threads=8, where='host'):
        """Index `files` (names relative to `root`) with `threads` <= 16 host threads of THIS process.  where='device': the
        threads read the files and their markers, the scans are walked on the device in batches (`index_jpeg_device`) and the
        rows read back; a file the device refuses goes through the host indexer, so every array equals the host build's."""
        from .. import _native as N
        N.lib()                                     # (load it once, before the threads ask for it)
        threads = max(1, min(int(threads), 16))
        if where not in ('host', 'device'):
            raise ValueError(f"where={where!r}: 'host' or 'device'")
        if where == 'device':
            return cls._build_device(files, root, seg_mcus, threads)

        def one(name):
            path = os.path.join(str(root), name)
            st = os.stat(path)
            rc, info, segs = index_jpeg(np.fromfile(path, np.uint8), seg_mcus)
            return info, segs, st.st_size, st.st_mtime_ns, _reason(rc, info)
        with ThreadPoolExecutor(max_workers=threads) as ex:
            return cls._from_rows(files, list(ex.map(one, files)), seg_mcus)

    @classmethod
    def _from_rows(cls, files, rows, seg_mcus):
        """rows: (info, segs, size, mtime_ns, reason) of each file -> the index of the flat arrays."""
        infos = np.array([r[0] for r in rows], INFO_DTYPE).reshape(-1)
        seg_start = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.int64)
        segs = np.concatenate([r[1] for r in rows] + [np.zeros(0, SEG_DTYPE)])
        return cls(files, infos, segs, seg_start, np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64),
                   np.array([r[4] for r in rows], np.int64), seg_mcus)

    @classmethod
    def _build_device(cls, files, root, seg_mcus, threads):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("JpegIndex.build(where='device') needs a GPU and none is present: build with where='host'")

        def read(name):
            path = os.path.join(str(root), name)
            st = os.stat(path)
            data = np.fromfile(path, np.uint8)
            rc, info = read_jpeg_header(data, seg_mcus)
            return data, rc, info, st.st_size, st.st_mtime_ns
        rows = []
        with ThreadPoolExecutor(max_workers=threads) as ex:
            for b0 in range(0, len(files), _INDEX_BATCH):
                batch = list(ex.map(read, files[b0:b0 + _INDEX_BATCH]))
                good = [k for k, r in enumerate(batch) if r[1] == 0]
                done = {}
                if good:
                    infos, segs, seg_start, status = index_jpeg_device([batch[k][0] for k in good], seg_mcus)
                    infos = infos.cpu().numpy().view(INFO_DTYPE)
                    segs, status = segs.cpu().numpy().view(SEG_DTYPE), status.cpu().numpy()
                    for n, k in enumerate(good):
                        if status[n] == 0:
                            done[k] = (infos[n].copy(), segs[seg_start[n]:seg_start[n + 1]].copy(), 0)
                for k, (data, rc, info, size, mtime) in enumerate(batch):
                    if k in done:
                        info, segs, reason = done[k]
                    elif rc == 0:                       # the device refuses its scan: the host indexer says why, in its own words
                        rc, info, segs = index_jpeg(data, seg_mcus)
                        reason = _reason(rc, info)
                    else:
                        segs, reason = np.zeros(0, SEG_DTYPE), _reason(rc, info)
                    rows.append((info, segs, size, mtime, reason))
        return cls._from_rows(files, rows, seg_mcus)

    def rows(self, i):
        """-> (info record, segment table) of file i: what `decode_jpeg_batch` takes."""
        return self.infos[i], self.segs[self.seg_start[i]:self.seg_start[i + 1]]

    def check(self, root, i=None):
        """Raises RuntimeError naming the first file (or file i) whose size or mtime is no longer what was indexed."""
        for k in (range(len(self.files)) if i is None else [i]):
            path = os.path.join(str(root), self.files[k])
            st = os.stat(path)
            if st.st_size != int(self.size[k]) or st.st_mtime_ns != int(self.mtime_ns[k]):
                raise RuntimeError(f'{path} changed since it was indexed (size {st.st_size} / mtime {st.st_mtime_ns} now, '
                                   f'{int(self.size[k])} / {int(self.mtime_ns[k])} in the index): rebuild the index')

    # ---- one flat uint8 array on disk: .npy (loadable with mmap_mode='r') or .npz ----
    def _sections(self):
        names = np.frombuffer('\n'.join(self.files).encode(), np.uint8)
        return [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in
                (self.infos, self.segs, self.seg_start, self.size, self.mtime_ns, self.reason, names)]

    def save(self, path):
        sec = self._sections()
        head = np.array([_MAGIC, len(self.files), len(self.segs), self.seg_mcus, sec[-1].size, 0, 0, 0], np.int64)
        parts, off = [head.view(np.uint8)], 64
        for s in sec:
            pad = -s.size % 64
            parts += [s, np.zeros(pad, np.uint8)]
            off += s.size + pad
        blob = np.concatenate(parts)
        path = str(path)
        if path.endswith('.npz'):
            np.savez(path, index=blob)
        else:
            with open(path, 'wb') as f:             # (np.save would append '.npy' to another suffix)
                np.save(f, blob)

    @classmethod
    def load(cls, path, mmap_mode=None):
        path = str(path)
        blob = np.load(path)['index'] if path.endswith('.npz') else np.load(path, mmap_mode=mmap_mode)
        head = np.asarray(blob[:64]).view(np.int64)
        if blob.dtype != np.uint8 or int(head[0]) != _MAGIC:
            raise RuntimeError(f'{path} is not a JPEG index')
        n, total, seg_mcus, nb = (int(v) for v in head[1:5])
        out, off = [], 64
        for dt, cnt in ((INFO_DTYPE, n), (SEG_DTYPE, total), (np.int64, n + 1), (np.int64, n), (np.int64, n), (np.int64, n),
                        (np.uint8, nb)):
            size = np.dtype(dt).itemsize * cnt
            out.append(blob[off:off + size].view(dt))
            off += size + -size % 64
        files = bytes(np.asarray(out[6])).decode().split('\n') if n else []
        return cls(files, *out[:6], seg_mcus)


def collate_jpeg(items):
    """DataLoader collate of `ObjectronFrames(decode='device')` items (payload, boxes, labels, i): the payloads -- file bytes, or
    a host-decoded frame for a file the index keeps on the host -- in one uint8 buffer with a table.
    -> (blob uint8 [bytes], table int64 [B, 5] = (dataset index, 0 bytes / 1 frame, offset in blob, bytes or h, 0 or w),
    boxes float32 [sum n, 4], labels int32 [sum n], counts int64 [B])."""
    import torch
    table = np.zeros((len(items), 5), np.int64)
    off = 0
    for k, (p, _, _, i) in enumerate(items):
        table[k] = (i, 1, off, p.shape[0], p.shape[1]) if p.ndim == 3 else (i, 0, off, p.size, 0)
        off += p.size
    blob = np.empty(max(off, 1), np.uint8)
    for (p, _, _, _), row in zip(items, table):
        blob[row[2]:row[2] + p.size] = p.reshape(-1)
    boxes = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for _, b, _, _ in items])
    labels = np.concatenate([np.asarray(l, np.int32).reshape(-1) for _, _, l, _ in items])
    counts = np.asarray([len(l) for _, _, l, _ in items], np.int64)
    return (torch.from_numpy(blob), torch.from_numpy(table), torch.from_numpy(boxes), torch.from_numpy(labels),
            torch.from_numpy(counts))


def _checked_infos(rows):
    """rows [(info, segs)] -> their info records as one array; ValueError for a row the device does not decode."""
    infos = np.array([r[0] for r in rows], INFO_DTYPE).reshape(-1)
    for inf, (_, s) in zip(infos, rows):
        if int(inf['reason']) or int(inf['nseg']) != len(s) or int(inf['nseg']) < 1:
            raise ValueError('an index row of a file the device does not decode (its reason is set, or its table is incomplete)')
    return infos


def plan_batch(rows, file_offsets, file_sizes, out_offsets):
    """The tables of one t3d_jpeg_decode_u8 call: rows [(info, segs)] of the batch's files, where each file's bytes lie in
    the data buffer and where its frame goes.  -> dict(infos, segs, items (numpy, to upload), total_segs, total_blocks,
    max_segs, max_blocks)."""
    infos = _checked_infos(rows)
    segs = np.concatenate([np.asarray(r[1]) for r in rows] + [np.zeros(0, SEG_DTYPE)])
    blocks = frame_blocks(infos)
    items = item_table(file_offsets, file_sizes, out_offsets, starts(infos['nseg']), blocks)
    return dict(infos=infos, segs=segs, items=items, total_segs=len(segs), total_blocks=int(blocks.sum()),
                max_segs=int(infos['nseg'].max()), max_blocks=int(blocks.max()))


def _launch(entry, B, data, infos, segs, tables, plan, out, bounds):
    """Workspace and status vector of one decode call over B items, then the call on the current stream.  tables: the device
    tensors between `segs` and `out` in the entry's argument list; bounds: the plan's keys of the entry's grid bounds.
    -> status, int32 [B]."""
    import ctypes

    import torch

    from .. import _native as N
    nbytes = ctypes.c_longlong(0)
    if N.lib().t3d_jpeg_decode_work_bytes(plan['total_blocks'], ctypes.byref(nbytes)) != 0:
        raise RuntimeError('t3d_jpeg_decode_work_bytes failed')
    work = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=out.device)
    status = torch.empty(max(B, 1), dtype=torch.int32, device=out.device)
    N.call(entry, N.ptr(data), data.numel(), N.ptr(infos), N.ptr(segs), plan['total_segs'], *[N.ptr(t) for t in tables], N.ptr(out),
           out.numel(), N.ptr(work), work.numel(), plan['total_blocks'], N.ptr(status), B, *[plan[k] for k in bounds], N.stream())
    return status[:B]


def launch_decode(data, infos, segs, items, plan, out):
    """Enqueue t3d_jpeg_decode_u8 on the current stream.  data, out: device uint8 tensors; infos, segs, items: device uint8
    tensors holding the B items' t3d_jpeg_info records, the segment rows their `seg_offset` points into and their t3d_jpeg_item
    table (`plan_batch`: plan['infos'], ['segs'], ['items']); plan: total_segs (rows in `segs`), total_blocks, max_segs,
    max_blocks.  -> status, device int32 [B] (0: decoded to the last MCU)."""
    return _launch('t3d_jpeg_decode_u8', items.numel() // ITEM_DTYPE.itemsize, data, infos, segs, (items,), plan, out,
                   ('max_segs', 'max_blocks'))


def _packed(sizes, dev):
    """[(h, w)] -> (device uint8 buffer for the RGB images one behind the other, desc int64 [B, 3] = (offset, h, w))."""
    import torch
    desc = np.zeros((len(sizes), 3), np.int64)
    desc[:, 1:] = np.asarray(sizes, np.int64).reshape(-1, 2)
    nb = desc[:, 1] * desc[:, 2] * 3
    desc[:, 0] = np.cumsum(nb) - nb
    dev = torch.device('cuda', torch.cuda.current_device()) if dev is None else torch.device(dev)
    return torch.empty(max(int(nb.sum()), 1), dtype=torch.uint8, device=dev), desc


def _upload_parts(parts, dev):
    """numpy uint8 arrays -> their device views inside ONE uploaded buffer (`pack`), through pageable memory: the upload has
    run when this returns, which the one-call forms below rely on."""
    import torch
    offs, total = pack(parts)
    host = np.zeros(max(total, 16), np.uint8)
    for p, o in zip(parts, offs):
        host[o:o + p.size] = p
    d = torch.from_numpy(host).to(dev)
    return [d[o:o + p.size] for p, o in zip(parts, offs)]


def decode_jpeg_batch(files, rows, device=None):
    """files: the contents of B JPEG files (bytes or uint8 arrays); rows: their index rows, [(info, segs)] from `JpegIndex.rows`
    or `index_jpeg` -> (packed device uint8 [sum h * w * 3], desc int64 [B, 3] = (offset, h, w)): the frames as RGB [h][w][3],
    the buffer and table `collate_frames` produces.  One t3d_jpeg_decode_u8 call on the current stream; nothing is read back
    (`decode_jpeg_batch.last_status` holds the call's device status vector)."""
    out, desc = _packed([(int(inf['h']), int(inf['w'])) for inf, _ in rows], device)
    if not len(files):
        return out, desc
    arrs = [np.frombuffer(f, np.uint8) for f in files]
    sizes = np.array([a.size for a in arrs], np.int64)
    plan = plan_batch(rows, np.cumsum(sizes) - sizes, sizes, desc[:, 0])
    parts = _upload_parts([np.concatenate(arrs)] + [plan[k].view(np.uint8) for k in ('infos', 'segs', 'items')], out.device)
    decode_jpeg_batch.last_status = launch_decode(*parts, plan, out)
    return out, desc


decode_jpeg_batch.last_status = None


# ---- the index built on the device: t3d_jpeg_index_device -------------------------------------------------------------------------
def _index_device(files, seg_mcus, sub_bytes, device, decode=False):
    """Headers on the host, ONE upload, ONE t3d_jpeg_index_device call on the current stream.  -> dict(data, infos, segs, items
    (device uint8 tensors; items: the DECODE's table when `decode`), status (device int32 [B]), seg_start (host int64 [B + 1]),
    heads (the host's header records), plan (what `launch_decode` takes), work (the call's workspace, settle rounds included))."""
    import ctypes

    import torch

    from .. import _native as N
    lo, hi = SUB_BYTES_RANGE
    sub_bytes = int(sub_bytes)
    if not lo <= sub_bytes <= hi:
        raise ValueError(f'sub_bytes={sub_bytes}: {lo} .. {hi}')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    arrs = [np.frombuffer(f, np.uint8) for f in files]
    heads = np.zeros(len(arrs), INFO_DTYPE)
    for i, a in enumerate(arrs):
        rc, heads[i] = read_jpeg_header(a, seg_mcus)
        if rc != 0:
            raise ValueError(f'file {i} of the batch is not decoded on the device: {REASONS[_reason(rc, heads[i])]}')
    B = len(arrs)
    sizes = np.array([a.size for a in arrs], np.int64)
    nseg = heads['nseg'].astype(np.int64)
    seg_start = np.concatenate([[0], np.cumsum(nseg)]).astype(np.int64)
    status = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    if B == 0:
        empty = torch.empty(0, dtype=torch.uint8, device=dev)
        return dict(data=empty, infos=empty, segs=empty, items=empty, status=status[:0], seg_start=seg_start, heads=heads, plan=None,
                    work=empty)
    nsub = -(-heads['scan_bytes'].astype(np.int64) // sub_bytes)
    blocks = frame_blocks(heads)
    items = item_table(starts(sizes), sizes, 0, seg_start[:-1], nsub)      # block_offset: subsequence records
    parts = [np.concatenate(arrs), heads.view(np.uint8), items.view(np.uint8)]
    if decode:
        frame_bytes = heads['h'].astype(np.int64) * heads['w'] * 3
        ditems = item_table(items['file_offset'], sizes, starts(frame_bytes), seg_start[:-1], blocks)
        parts.append(ditems.view(np.uint8))
    parts = _upload_parts(parts, dev)
    total_segs = int(seg_start[-1])
    segs = torch.empty(total_segs * SEG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    nbytes = ctypes.c_longlong(0)
    if N.lib().t3d_jpeg_index_work_bytes(int(heads['scan_bytes'].sum()), B, sub_bytes, ctypes.byref(nbytes)) != 0:
        raise RuntimeError('t3d_jpeg_index_work_bytes failed')
    work = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dev)
    N.call('t3d_jpeg_index_device', N.ptr(parts[0]), parts[0].numel(), N.ptr(parts[1]), N.ptr(segs), total_segs, N.ptr(parts[2]), sub_bytes,
           N.ptr(work), work.numel(), N.ptr(status), B, int(nsub.max()), N.stream())
    plan = dict(total_segs=total_segs, total_blocks=int(blocks.sum()), max_segs=int(nseg.max()), max_blocks=int(blocks.max()))
    return dict(data=parts[0], infos=parts[1], segs=segs, items=parts[-1], status=status[:B], seg_start=seg_start, heads=heads, plan=plan,
                work=work)


def index_jpeg_device(files, seg_mcus=DEFAULT_SEG_MCUS, sub_bytes=DEFAULT_SUB_BYTES, device=None):
    """files: the contents of B JPEG files nobody has indexed -> (infos, segs, seg_start, status): the index rows built on the
    device.  infos: device uint8 [B * 864] (INFO_DTYPE records), segs: device uint8 [total * 16] (SEG_DTYPE rows), file i's from
    seg_start[i] (host int64 [B + 1]) on, status: device int32 [B] -- 0: the rows and scan_bytes are `index_jpeg`'s, byte for
    byte; 1: a scan the host indexer calls malformed (its scan_bytes is -1: a decode given the record refuses the image).
    The markers are read on the host; then one upload and one t3d_jpeg_index_device call on the current stream, nothing is read
    back.  ValueError: a file whose markers the device path does not take, naming its reason from REASONS."""
    d = _index_device(files, seg_mcus, sub_bytes, device)
    return d['infos'], d['segs'], d['seg_start'], d['status']


def decode_jpeg_frames(files, device=None, seg_mcus=DEFAULT_SEG_MCUS, sub_bytes=DEFAULT_SUB_BYTES):
    """files: the contents of B JPEG files nobody has indexed -> (packed device uint8 [sum h * w * 3], desc int64 [B, 3] =
    (offset, h, w)), the layout of `decode_jpeg_batch`.  t3d_jpeg_index_device and t3d_jpeg_decode_u8 back to back on the
    current stream: no host scan walk, nothing read back.  `decode_jpeg_frames.last_status` = (the indexer's, the decode's)
    device status vectors: a frame whose scan the indexer refuses (1) is refused by the decode (2) and its pixels are not written."""
    d = _index_device(files, seg_mcus, sub_bytes, device, decode=True)
    out, desc = _packed([(int(h['h']), int(h['w'])) for h in d['heads']], d['status'].device)
    if not len(files):
        return out, desc
    decode_jpeg_frames.last_status = (d['status'], launch_decode(d['data'], d['infos'], d['segs'], d['items'], d['plan'], out))
    return out, desc


decode_jpeg_frames.last_status = None


# ---- one pixel rectangle per file: t3d_jpeg_decode_roi_u8 ---------------------------------------------------------------------
def roi_mcus(sampling, h, w, x0, y0, x1, y1):
    """The MCU rectangle (mx0, my0, mx1, my1) holding every block the full decode reads for the pixels [x0, x1) x [y0, y1) of an
    h x w image (include/t3d.h next to t3d_jpeg_decode_roi_u8; csrc/jpeg_decode.h: roi_mcus).  Gray / 4:4:4: the pixels' MCUs.
    4:2:0: fancy upsampling of pixel (y, x) also reads chroma row (y >> 1) - 1 (y even) or + 1 (y odd) and chroma column
    (x >> 1) - 1 (x even) or + 1 (x odd), clamped to the real samples; for dw <= 2 libjpeg replicates and reads no neighbour."""
    if not (0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h):
        raise ValueError(f'the rectangle [{x0}, {x1}) x [{y0}, {y1}) is empty or outside the {h} x {w} image')
    if sampling != 2:
        return x0 >> 3, y0 >> 3, ((x1 - 1) >> 3) + 1, ((y1 - 1) >> 3) + 1
    dh, dw = (h + 1) >> 1, (w + 1) >> 1
    cx0, cx1, cy0, cy1 = x0 >> 1, (x1 - 1) >> 1, y0 >> 1, (y1 - 1) >> 1          # chroma samples, inclusive
    if dw > 2:
        if not x0 & 1:
            cx0 = max(cx0 - 1, 0)
        if (x1 - 1) & 1:
            cx1 = min(cx1 + 1, dw - 1)
        if not y0 & 1:
            cy0 = max(cy0 - 1, 0)
        if (y1 - 1) & 1:
            cy1 = min(cy1 + 1, dh - 1)
    return cx0 >> 3, cy0 >> 3, (cx1 >> 3) + 1, (cy1 >> 3) + 1


def plan_roi(info, segs, x0, y0, x1, y1):
    """Pure numpy: what decoding the pixels [x0, x1) x [y0, y1) of one indexed file takes.  info, segs: the file's index rows
    (`JpegIndex.rows`; segs may be a memory map -- only two of its entries are read).  -> dict:
      rect (x0, y0, x1, y1);  mcus (mx0, my0, mx1, my1), `roi_mcus`
      row_segs int64 [my1 - my0, 2]: MCU row my0 + r needs the segments row_segs[r, 0] .. row_segs[r, 1] - 1; a segment that
                 straddles rows is listed in the first row that needs it, so every needed segment appears once
      seg_first, seg_count: the contiguous run of the file's segments from the first needed to the last needed one
      span (first, bytes): the bytes of the SCAN (offsets from info['scan_offset']) from the first needed segment's byte to the
                 byte of the segment behind the last needed one plus ROI_READ_AHEAD, or to the scan's end
      blocks: 8x8 blocks of the MCU rectangle;  lanes, runs: the item's share of the call's grid bounds."""
    h, w, S, X = int(info['h']), int(info['w']), int(info['seg_mcus']), int(info['mcus_x'])
    x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
    mx0, my0, mx1, my1 = roi_mcus(int(info['sampling']), h, w, x0, y0, x1, y1)
    if my1 - my0 <= 8:                               # (a handful of rows: faster without numpy)
        b = [(my * X + mx1 - 1) // S for my in range(my0, my1)]
        a = [max((my * X + mx0) // S, b[r - 1] + 1 if r else 0) for r, my in enumerate(range(my0, my1))]
        row_segs = np.array([(u, max(v + 1, u)) for u, v in zip(a, b)], np.int64)
    else:
        base = np.arange(my0, my1, dtype=np.int64) * X
        a, b = (base + mx0) // S, (base + mx1 - 1) // S
        a[1:] = np.maximum(a[1:], b[:-1] + 1)
        row_segs = np.stack([a, np.maximum(b + 1, a)], 1)
    s_lo, s_hi = int(a[0]), int(b[-1])
    first = int(segs[s_lo]['byte'])
    scan_bytes = int(info['scan_bytes'])
    end = min(int(segs[s_hi + 1]['byte']) + ROI_READ_AHEAD, scan_bytes) if s_hi + 1 < int(info['nseg']) else scan_bytes
    rw, rh = mx1 - mx0, my1 - my0
    return dict(rect=(x0, y0, x1, y1), mcus=(mx0, my0, mx1, my1), row_segs=row_segs, seg_first=s_lo, seg_count=s_hi - s_lo + 1,
                span=(first, end - first), blocks=rw * rh * int(mcu_blocks(info['sampling'])),
                lanes=rh * ((rw - 1) // S + 2), runs=(y1 - y0) * ((x1 - x0 + 3) // 4))


def plan_roi_batch(rows, plans, data_offsets, out_offsets, spans=None):
    """The tables of one t3d_jpeg_decode_roi_u8 call.  rows [(info, segs)] and plans [`plan_roi`] of the batch's items;
    data_offsets: where each item's uploaded scan bytes lie in the data buffer; spans [(first, bytes)]: which bytes of the scan
    those are (None: each plan's own span); out_offsets: where each crop goes.
    -> dict(infos, segs, items, rects (numpy, to upload), total_segs, total_blocks, max_lanes, max_blocks, max_runs)."""
    infos = _checked_infos(rows)
    segs = np.concatenate([np.asarray(r[1][p['seg_first']:p['seg_first'] + p['seg_count']]) for r, p in zip(rows, plans)]
                          + [np.zeros(0, SEG_DTYPE)])
    spans = [p['span'] for p in plans] if spans is None else spans
    nseg = np.array([p['seg_count'] for p in plans], np.int64)
    blocks = np.array([p['blocks'] for p in plans], np.int64)
    items = item_table(data_offsets, [s[1] for s in spans], out_offsets, starts(nseg), blocks)
    items['reserved'] = [s[0] for s in spans]
    rects = np.zeros((len(rows), 12), np.int32)
    for k, p in enumerate(plans):
        rects[k, :10] = p['rect'] + p['mcus'] + (p['seg_first'], p['seg_count'])
    return dict(infos=infos, segs=segs, items=items, rects=rects, total_segs=len(segs), total_blocks=int(blocks.sum()),
                max_lanes=max(p['lanes'] for p in plans), max_blocks=int(blocks.max()), max_runs=max(p['runs'] for p in plans))


def launch_decode_roi(data, infos, segs, items, rects, plan, out):
    """Enqueue t3d_jpeg_decode_roi_u8 on the current stream.  data, out: device uint8 tensors; infos, segs, items, rects: device
    uint8 tensors holding plan['infos'], ['segs'], ['items'], ['rects'] (`plan_roi_batch`).  -> status, device int32 [B]."""
    return _launch('t3d_jpeg_decode_roi_u8', items.numel() // ITEM_DTYPE.itemsize, data, infos, segs, (items, rects), plan, out,
                   ('max_lanes', 'max_blocks', 'max_runs'))


def decode_jpeg_rois(files, rows, rects, device=None, partial=True):
    """files: the contents of B JPEG files; rows: their index rows; rects [B] (x0, y0, x1, y1) -> (packed device uint8
    [sum h * w * 3], desc int64 [B, 3] = (offset, h, w)): the rectangles as RGB, the buffer and table `collate_crops` produces
    for the sliced frames.  partial: upload each file's planned byte span only (else its whole scan).  One
    t3d_jpeg_decode_roi_u8 call on the current stream; `decode_jpeg_rois.last_status` holds its device status vector."""
    out, desc = _packed([(y1 - y0, x1 - x0) for x0, y0, x1, y1 in rects], device)
    if not len(files):
        return out, desc
    plans = [plan_roi(inf, sg, *r) for (inf, sg), r in zip(rows, rects)]
    spans = [p['span'] if partial else (0, int(inf['scan_bytes'])) for p, (inf, _) in zip(plans, rows)]
    arrs = [np.frombuffer(f, np.uint8)[int(inf['scan_offset']) + a:int(inf['scan_offset']) + a + n]
            for f, (inf, _), (a, n) in zip(files, rows, spans)]
    sizes = np.array([a.size for a in arrs], np.int64)
    plan = plan_roi_batch(rows, plans, np.cumsum(sizes) - sizes, desc[:, 0], spans)
    parts = _upload_parts([np.concatenate(arrs)] + [plan[k].reshape(-1).view(np.uint8) for k in ('infos', 'segs', 'items', 'rects')],
                          out.device)
    decode_jpeg_rois.last_status = launch_decode_roi(*parts, plan, out)
    return out, desc


decode_jpeg_rois.last_status = None

