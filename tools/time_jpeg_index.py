"""Cost of the MCU index built on the device (csrc/jpeg_scan.hip, dataloaders/jpeg.py: index_jpeg_device) beside the host scan
walk it replaces (t3d_jpeg_index), on one GPU.

Frames from the generator of tools/time_jpeg_decode.py (a smooth random field plus noise, quality 90, 4:2:0): B = 80 at
1440 x 1920, B = 1 and 8 at 1080 x 1920.  Device-event times, 5 warm-up calls, then the median and min-max of --reps.  One JSON
line per measurement:
  1. `t3d_jpeg_index_device` alone for sub_bytes 4, 8, .. 512, its rows checked against the host indexer's, with the settle rounds
     the frames took;
  2. index + `t3d_jpeg_decode_u8` back to back at the best sub_bytes of the sweep;
  3. `t3d_jpeg_decode_u8` with a prebuilt index: the control, its code is unchanged;
  4. the host `t3d_jpeg_index` over the same files on 1 and 8 threads (wall clock, median of 5);
  5. the verdict: the device path against the host index on 8 threads plus the decode -- a gain where its median is below by more
     than the sum of the two spreads;
  6. the settle rounds of whatever real JPEG files the Python packages of this machine carry (the generated frames do not show what
     photographs need).
`--index-only SUB` runs only 5 + --reps index calls at B = 80: the run to put under a kernel trace for the per-kernel split.
Usage: python tools/time_jpeg_index.py [--reps 50] [--index-only SUB] [--out FILE]"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import time_jpeg_decode as T  # noqa: E402

SWEEP = (4, 8, 16, 32, 64, 128, 256, 512)
SEG = 2


def frames(B, h, w):
    T.H, T.W = h, w
    return [T.frame_jpeg(i) for i in range(B)]


class Index:
    """The device side of one t3d_jpeg_index_device call over `files`, headers and tables uploaded once.  (The call does not read
    scan_bytes, the one field it writes, so it may run again on its own output.)"""

    def __init__(self, files, sub, seg_mcus=SEG):
        import ctypes

        from torchdet3d import _native as N
        from torchdet3d.dataloaders import jpeg as J
        self.N, self.J, self.sub, self.B = N, J, sub, len(files)
        heads = np.zeros(len(files), J.INFO_DTYPE)
        for i, f in enumerate(files):
            rc, heads[i] = J.read_jpeg_header(f, seg_mcus)
            assert rc == 0
        sizes = np.array([len(f) for f in files], np.int64)
        nseg, self.nsub = heads['nseg'].astype(np.int64), -(-heads['scan_bytes'].astype(np.int64) // sub)
        blocks = heads['mcus_x'].astype(np.int64) * heads['mcus_y'] * np.asarray((1, 3, 6), np.int64)[heads['sampling']]
        frame = heads['h'].astype(np.int64) * heads['w'] * 3
        items = np.zeros(len(files), J.ITEM_DTYPE)
        items['file_offset'], items['file_bytes'] = np.cumsum(sizes) - sizes, sizes
        items['seg_offset'], items['block_offset'] = np.cumsum(nseg) - nseg, np.cumsum(self.nsub) - self.nsub
        ditems = items.copy()
        ditems['out_offset'], ditems['block_offset'] = np.cumsum(frame) - frame, np.cumsum(blocks) - blocks
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()      # noqa: E731
        self.data, self.infos, self.items, self.ditems = up(np.frombuffer(b''.join(files), np.uint8)), up(heads), up(items), up(ditems)
        self.total = int(nseg.sum())
        self.segs = torch.empty(self.total * 16, dtype=torch.uint8, device='cuda')
        nb = ctypes.c_longlong(0)
        assert N.lib().t3d_jpeg_index_work_bytes(int(heads['scan_bytes'].sum()), self.B, sub, ctypes.byref(nb)) == 0
        self.work = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
        self.status = torch.empty(self.B, dtype=torch.int32, device='cuda')
        self.out = torch.empty(int(frame.sum()), dtype=torch.uint8, device='cuda')
        self.plan = dict(infos=heads, total_segs=self.total, total_blocks=int(blocks.sum()), max_segs=int(nseg.max()), max_blocks=int(blocks.max()))

    def __call__(self):
        N = self.N
        N.call('t3d_jpeg_index_device', N.ptr(self.data), self.data.numel(), N.ptr(self.infos), N.ptr(self.segs), self.total, N.ptr(self.items),
               self.sub, N.ptr(self.work), self.work.numel(), N.ptr(self.status), self.B, int(self.nsub.max()), N.stream())

    def decode(self):
        self.dstatus = self.J.launch_decode(self.data, self.infos, self.segs, self.ditems, self.plan, self.out)

    def both(self):
        self()
        self.decode()

    def rounds(self):
        return self.work[:32 * self.B].cpu().numpy().view(np.int32).reshape(self.B, 8)[:, 1]

    def equals(self, rows):
        J = self.J
        ok = not self.status.any().item()
        ok = ok and self.segs.cpu().numpy().tobytes() == np.concatenate([r[2] for r in rows]).tobytes()
        return ok and self.infos.cpu().numpy().tobytes() == np.array([r[1] for r in rows], J.INFO_DTYPE).tobytes()


def host_index(files, threads, reps=5):
    from torchdet3d.dataloaders import jpeg as J
    J.index_jpeg(files[0], SEG)
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        if threads == 1:
            for f in files:
                J.index_jpeg(f, SEG)
        else:
            with ThreadPoolExecutor(max_workers=threads) as ex:
                list(ex.map(lambda f: J.index_jpeg(f, SEG), files))
        s.append(time.perf_counter() - t0)
    return s


def real_files(limit=40):
    """JPEG files that come with the Python packages of this machine (test images of Pillow, torch, ...), smallest first."""
    found = []
    for root in {p for p in sys.path if p.endswith('-packages') and os.path.isdir(p)}:
        for d, _, names in os.walk(root):
            found += [os.path.join(d, n) for n in names if n.lower().endswith(('.jpg', '.jpeg'))]
    return sorted(set(found), key=os.path.getsize)[:limit]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--index-only', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from torchdet3d.dataloaders import jpeg as J

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    if a.index_only:
        ix = Index(frames(80, 1440, 1920), a.index_only)
        T.timed(ix, a.reps)
        assert not ix.status.any().item()
        return
    for B, h, w in ((80, 1440, 1920), (1, 1080, 1920), (8, 1080, 1920)):
        files = frames(B, h, w)
        rows = [J.index_jpeg(f, SEG) for f in files]
        emit(what='the generated frames', B=B, frame=[h, w], quality=90, sampling='4:2:0', jpeg_bytes_mean=int(np.mean([len(f) for f in files])))
        best = None
        for sub in SWEEP:
            ix = Index(files, sub)
            ms = T.timed(ix, a.reps)
            r = ix.rounds()
            emit(what='t3d_jpeg_index_device, one call over the batch', B=B, frame=[h, w], sub_bytes=sub, lanes_per_frame=int(ix.nsub.max()),
                 equals_host_rows=ix.equals(rows), settle_rounds_median=int(np.median(r)), settle_rounds_max=int(r.max()), **T.stats(ms))
            if best is None or np.median(ms) < best[1]:
                best = (sub, float(np.median(ms)))
            del ix
        emit(what='best sub_bytes of the sweep', B=B, frame=[h, w], sub_bytes=best[0], median_us=round(best[1] * 1e3, 1), default=J.DEFAULT_SUB_BYTES)
        ix = Index(files, best[0])
        both = T.timed(ix.both, a.reps)
        want = np.asarray(Image.open(io.BytesIO(files[0])).convert('RGB'))
        ok = not ix.dstatus.any().item() and bool((ix.out[:want.size].cpu().numpy().reshape(want.shape) == want).all())
        emit(what='index + decode back to back', B=B, frame=[h, w], sub_bytes=best[0], seg_mcus=SEG, equals_pillow=ok, **T.stats(both))
        ix()
        dec = T.timed(ix.decode, a.reps)
        emit(what='t3d_jpeg_decode_u8 with a prebuilt index (the control)', B=B, frame=[h, w], seg_mcus=SEG, **T.stats(dec))
        host = {t: host_index(files, t) for t in (1, 8)}
        for t, s in host.items():
            emit(what='host t3d_jpeg_index over the same files', B=B, frame=[h, w], threads=t, median_ms=round(float(np.median(s)) * 1e3, 2),
                 min_ms=round(min(s) * 1e3, 2), max_ms=round(max(s) * 1e3, 2), files_per_s=round(B / float(np.median(s)), 1))
        parent = float(np.median(host[8])) * 1e3 + float(np.median(dec))
        spread = (max(host[8]) - min(host[8])) * 1e3 + (max(dec) - min(dec)) + (max(both) - min(both))
        emit(what='verdict: device index + decode against host index on 8 threads + decode', B=B, frame=[h, w],
             device_path_median_ms=round(float(np.median(both)), 3), parent_path_median_ms=round(parent, 3), sum_of_spreads_ms=round(spread, 3),
             gain=bool(parent - float(np.median(both)) > spread))
        del ix
    found = real_files()
    if not found:
        emit(what='real JPEG files on this machine', found=0)
    for path in found:
        data = open(path, 'rb').read()
        rc, info = J.read_jpeg_header(data, SEG)
        if rc != 0:
            emit(what='a real JPEG file', file=os.path.basename(path), bytes=len(data), taken=False, reason=J.REASONS[int(info['reason']) if rc == -3 else -1])
            continue
        for sub in (16, 64, 256):
            ix = Index([data], sub)
            ix()
            torch.cuda.synchronize()
            emit(what='a real JPEG file', file=os.path.basename(path), bytes=len(data), size=[int(info['h']), int(info['w'])], sub_bytes=sub,
                 lanes=int(ix.nsub.max()), settle_rounds=int(ix.rounds()[0]), status=int(ix.status[0].item()),
                 host_return_code=int(J.index_jpeg(data, SEG)[0]))


if __name__ == '__main__':
    main()
