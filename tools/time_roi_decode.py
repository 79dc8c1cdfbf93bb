"""Cost of the rectangle decode (t3d_jpeg_decode_roi_u8: csrc/jpeg.hip, dataloaders/jpeg.py) beside the full-frame device decode,
on one GPU.

B = 164 generated frames of 1440 x 1920 (the generator of tools/time_jpeg_decode.py: quality 90, 4:2:0) with one seeded box each
-- width and height uniform in 15 .. 60 % of the frame's, placed uniformly; the distribution of the boxes' share of the frame
is the first output line.  One JSON line per measurement:
  1. device-event time of one `t3d_jpeg_decode_roi_u8` call over the B boxes (5 warm-up calls, then --reps timed: median, min,
     max) with the planned byte spans uploaded, for seg_mcus in 1, 2, 4, 8, 16, and the bytes the call needs uploaded;
  2. the same for one `t3d_jpeg_decode_u8` call over the same B frames at its default seg_mcus: the yardstick;
`--decode-only SEG` runs only 5 + --reps rectangle calls at one seg_mcus and `--decode-only-full` only the full-frame calls: the
runs to put under `rocprofv3 --kernel-trace --stats`; `--kernel-stats CSV` copies the jpeg kernels' rows of such a run's
kernel_stats file into the output.
Usage: python tools/time_roi_decode.py [--batch 164] [--reps 50] [--parts decode,full] [--out FILE]"""
import argparse
import csv
import io
import json
import os
import re
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from time_jpeg_decode import Decode, H, W, frame_jpeg, stats, timed  # noqa: E402

SWEEP = (1, 2, 4, 8, 16)


def boxes(n, seed=7):
    rng = np.random.default_rng(seed)
    bw, bh = (rng.uniform(.15, .6, n) * W).astype(int), (rng.uniform(.15, .6, n) * H).astype(int)
    x0, y0 = (rng.uniform(0, 1, n) * (W - bw)).astype(int), (rng.uniform(0, 1, n) * (H - bh)).astype(int)
    return [(int(a), int(b), int(a + c), int(b + d)) for a, b, c, d in zip(x0, y0, bw, bh)]


class RoiDecode:
    """The device side of one t3d_jpeg_decode_roi_u8 call over `files` and `rects`, spans and tables uploaded once."""

    def __init__(self, files, rects, seg_mcus):
        from torchdet3d.dataloaders import jpeg as J
        rows = [J.index_jpeg(f, seg_mcus) for f in files]
        assert all(r[0] == 0 for r in rows)
        rows = [r[1:] for r in rows]
        plans = [J.plan_roi(inf, sg, *r) for (inf, sg), r in zip(rows, rects)]
        spans = [np.frombuffer(f, np.uint8)[int(inf['scan_offset']) + p['span'][0]:int(inf['scan_offset']) + sum(p['span'])]
                 for f, (inf, _), p in zip(files, rows, plans)]
        sizes = np.array([s.size for s in spans], np.int64)
        crop = np.array([(r[3] - r[1]) * (r[2] - r[0]) * 3 for r in rects], np.int64)
        self.plan = J.plan_roi_batch(rows, plans, np.cumsum(sizes) - sizes, np.cumsum(crop) - crop)
        self.span_bytes = int(sizes.sum())
        self.table_bytes = sum(self.plan[k].nbytes for k in ('infos', 'segs', 'items', 'rects'))
        self.data = torch.from_numpy(np.concatenate(spans)).cuda()
        self.tabs = [torch.from_numpy(self.plan[k].reshape(-1).view(np.uint8).copy()).cuda() for k in ('infos', 'segs', 'items', 'rects')]
        self.out = torch.empty(int(crop.sum()), dtype=torch.uint8, device='cuda')
        self.first = int(crop[0])
        self.launch = J.launch_decode_roi

    def __call__(self):
        self.status = self.launch(self.data, *self.tabs, self.plan, self.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=164)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--decode-only', type=int, default=0)
    ap.add_argument('--decode-only-full', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--parts', default='decode,full', help='which measurements to run')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(lines[-1] + '\n')
    if a.kernel_stats:
        with open(a.kernel_stats) as f:
            for row in csv.DictReader(f):
                if 'jpeg' in row.get('Name', ''):
                    emit(what='kernel trace, one run of 5 + reps calls', kernel=re.search(r'jpeg_\w+', row['Name']).group(0), calls=int(row['Calls']),
                         average_us=round(float(row['AverageNs']) / 1e3, 1), min_us=round(float(row['MinNs']) / 1e3, 1),
                         max_us=round(float(row['MaxNs']) / 1e3, 1))
        return
    B = a.batch
    with ProcessPoolExecutor(16) as ex:             # (before the GPU is initialised: the children never see it)
        files = list(ex.map(frame_jpeg, range(B)))
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from torchdet3d.dataloaders.jpeg import DEFAULT_SEG_MCUS, ROI_SEG_MCUS
    rects = boxes(B)
    if a.decode_only or a.decode_only_full:
        d = Decode(files, DEFAULT_SEG_MCUS) if a.decode_only_full else RoiDecode(files, rects, a.decode_only)
        timed(d, a.reps)
        assert not d.status.any().item()
        return
    parts = a.parts.split(',')
    share = np.array([(r[2] - r[0]) * (r[3] - r[1]) / (H * W) for r in rects])
    emit(what='the generated frames and boxes', B=B, frame=[H, W], quality=90, sampling='4:2:0',
         jpeg_bytes_mean=int(np.mean([len(f) for f in files])), box_share_of_frame=dict(
             min=round(float(share.min()), 4), p25=round(float(np.percentile(share, 25)), 4), median=round(float(np.median(share)), 4),
             mean=round(float(share.mean()), 4), p75=round(float(np.percentile(share, 75)), 4), max=round(float(share.max()), 4)))
    from PIL import Image
    if 'decode' in parts:
        want = np.asarray(Image.open(io.BytesIO(files[0])).convert('RGB'))[rects[0][1]:rects[0][3], rects[0][0]:rects[0][2]]
        best = None
        for seg in SWEEP:
            d = RoiDecode(files, rects, seg)
            ms = timed(d, a.reps)
            ok = not d.status.any().item() and bool((d.out[:d.first].cpu().numpy().reshape(want.shape) == want).all())
            emit(what='t3d_jpeg_decode_roi_u8, one call over the batch', seg_mcus=seg, equals_pillow=ok, span_bytes_uploaded=d.span_bytes,
                 table_bytes_uploaded=d.table_bytes, blocks=d.plan['total_blocks'], **stats(ms))
            if best is None or np.median(ms) < best[1]:
                best = (seg, float(np.median(ms)), min(ms), max(ms))
            del d
        emit(what='best seg_mcus of the sweep', seg_mcus=best[0], median_us=round(best[1] * 1e3, 1), default=ROI_SEG_MCUS)
    if 'full' in parts:
        d = Decode(files, DEFAULT_SEG_MCUS)
        ms = timed(d, a.reps)
        emit(what='t3d_jpeg_decode_u8, one call over the same frames', seg_mcus=DEFAULT_SEG_MCUS, ok=not d.status.any().item(),
             file_bytes_uploaded=int(sum(len(f) for f in files)), table_bytes_uploaded=sum(d.plan[k].nbytes for k in ('infos', 'segs', 'items')),
             **stats(ms))
        if 'decode' in parts:
            emit(what='rectangle call against full decode', roi_median_us=round(best[1] * 1e3, 1), full_median_us=round(float(np.median(ms)) * 1e3, 1),
                 roi_below_full_by_more_than_both_spreads=bool(np.median(ms) - best[1] > (max(ms) - min(ms)) + (best[3] - best[2])))
        del d


if __name__ == '__main__':
    main()
